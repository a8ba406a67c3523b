// mrg_comm.h -- the RCCL side of the host layer: the communicator behind the opaque mrg_comm of include/mrgpu.h,
// and what mrg_run.cpp calls of mrg_exchange.cpp to make and to abort the communicators of one mrg_run_job.
// Private to those two units: every other unit of libmrgpu.so compiles without RCCL's header.
#pragma once
#include <rccl/rccl.h>

#include <atomic>

#include "mrg_host.h"

#define NCCLCHK(x)                                                                                 \
    do {                                                                                           \
        ncclResult_t r_ = (x);                                                                     \
        if (r_ != ncclSuccess) ::mrg_host::raise(MRG_ECOMM, "%s: %s", #x, ncclGetErrorString(r_)); \
    } while (0)

struct mrg_comm {
    ncclComm_t comm = nullptr;
    int n = 0, rank = 0, device = 0;
    // preallocated at init, so the exchange never allocates before a collective that its peers are
    // already waiting in: the counts message [3 * n send | 3 * n receive] and the status word
    uint64_t *d_counts = nullptr;
    int *d_flag = nullptr;
    std::atomic<bool> aborted{false};  // ncclCommAbort was called (by this rank or by mrg_run_job's watchdog)
    // held around every RCCL enqueue of a rank thread and around the abort, so mrg_run_job's watchdog
    // does not free the communicator (ncclCommAbort) between a rank thread's aborted-check and its
    // RCCL call; never held across a wait on the stream
    std::timed_mutex mu;
};

namespace mrg_host __attribute__((visibility("hidden"))) {

// ---- mrg_exchange.cpp
std::vector<mrg_comm *> comm_init_all(const std::vector<int> &devices);
void comm_abort(mrg_comm *m, std::chrono::steady_clock::time_point deadline);

}  // namespace mrg_host
