// mrg_exchange.cpp -- the shuffle: a job's keys as exchange records by owner
// (export_sizes, export_pack), received records back into keys (import_recs, job_import), the RCCL communicator
// (mrg_comm.h) with its abort protocol, the exchange itself (job_shuffle), and the entry points mrg_comm_* and
// mrg_job_shuffle.  The only unit that calls RCCL; mrg_run.cpp takes its communicators from comm_init_all.
// Calls: mrg_agg.cpp (acc_emit, wide_densify, acc_release, aggregate), mrg_map.cpp (read_counters).
// Called by: mrgpu.cpp (the mrg_job_export* / mrg_job_import wrappers), mrg_plugin.cpp, mrg_run.cpp.
// comm_alloc and comm_free have no caller outside this unit since comm_init_all took mrg_run_job's
// ncclCommInitAll block, and stay local; test_fail (MRG_TEST_FAIL) lives here because the exchange's stages use it.
#include "mrg_comm.h"

using namespace mrg_host;

static_assert(sizeof(XRec) == MRG_XREC_BYTES, "exchange record layout (include/mrgpu.h)");

namespace {

// A communicator shell with its preallocated exchange buffers (the RCCL communicator is added by
// the caller).
mrg_comm *comm_alloc(int device, int n, int rank) {
    HIPCHK(hipSetDevice(device));
    mrg_comm *m = new mrg_comm();
    m->n = n;
    m->rank = rank;
    m->device = device;
    if (hipMalloc(&m->d_counts, 48ull * (uint64_t)n) != hipSuccess || hipMalloc(&m->d_flag, 64) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(m->d_counts);
        delete m;
        raise(MRG_ENOMEM, "communicator buffers: device allocation failed");
    }
    return m;
}

void comm_free(mrg_comm *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipFree(m->d_counts);
    (void)hipFree(m->d_flag);
    delete m;
}

// An RCCL call of the exchange: on failure the communicator is aborted (its peers' pending operations
// then fail instead of waiting forever) and the call raises MRG_ECOMM.
// Caller holds m->mu (a CommLock).
void nccl_or_abort(mrg_comm *m, ncclResult_t r, const char *what) {
    if (r == ncclSuccess) return;
    if (!m->aborted.exchange(true)) (void)ncclCommAbort(m->comm);
    raise(MRG_ECOMM, "%s: %s (communicator aborted)", what, ncclGetErrorString(r));
}

void check_not_aborted(mrg_comm *m) {
    if (m->aborted.load()) raise(MRG_ECOMM, "the communicator was aborted (another rank of the job failed)");
}

// The communicator's lock for a run of RCCL enqueues, taken only if it has not been aborted (the
// abort frees it): a watchdog abort waits for the enqueues, and enqueues after it raise MRG_ECOMM.
struct CommLock {
    std::unique_lock<std::timed_mutex> lk;
    explicit CommLock(mrg_comm *m) : lk(m->mu) { check_not_aborted(m); }
};

// Max of `flag` over the ranks (one RCCL all-reduce into the preallocated status word): every rank
// learns whether any rank failed, so all of them leave the exchange together.
int agree(mrg_ctx *c, mrg_comm *m, int flag) {
    check_not_aborted(m);
    HIPCHK(hipMemcpyAsync(m->d_flag, &flag, sizeof flag, hipMemcpyHostToDevice, c->stream));
    {
        CommLock lk(m);
        nccl_or_abort(m, ncclAllReduce(m->d_flag, m->d_flag, 1, ncclInt, ncclMax, m->comm, c->stream), "ncclAllReduce");
    }
    int any = 0;
    HIPCHK(hipMemcpyAsync(&any, m->d_flag, sizeof any, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    check_not_aborted(m);
    return any;
}

// A pair of timing events, destroyed on every exit.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() {
        HIPCHK(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipEventDestroy(e0);
            raise(MRG_EHIP, "hipEventCreate failed");
        }
    }
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
};

// An RCCL call inside the send/recv group: on failure the group is closed first (the calling thread's
// group depth stays balanced for its next RCCL call), then the communicator is aborted.
void group_or_abort(mrg_comm *m, ncclResult_t r, const char *what) {
    if (r == ncclSuccess) return;
    (void)ncclGroupEnd();
    nccl_or_abort(m, r, what);
}

}  // namespace

namespace mrg_host __attribute__((visibility("hidden"))) {

void export_sizes(mrg_ctx *c, uint32_t n_owners, uint64_t *h_rec, uint64_t *h_heap) {
    need_job(c);
    if (!c->mapped) raise(MRG_EINVAL, "export before map");
    if (n_owners == 0) raise(MRG_EINVAL, "n_owners must be > 0");
    acc_emit(c);
    wide_densify(c, 0);
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    unsigned long long *d = sc.get<unsigned long long>(2ull * n_owners);
    HIPCHK(hipMemsetAsync(d, 0, 16ull * n_owners, s));
    c->xrec_vmax = std::max<uint64_t>(1, std::min<uint64_t>(MRG_XREC_VMAX, env_u64("MRG_TEST_XREC_VMAX", MRG_XREC_VMAX)));
    mrg_launch_export_count(c->keys.ks, c->keys.n, n_owners, d, d + n_owners, is_idx(c), c->xrec_vmax, s);
    std::vector<uint64_t> h(2ull * n_owners);
    HIPCHK(hipMemcpyAsync(h.data(), d, 16ull * n_owners, hipMemcpyDeviceToHost, s));
    sync(c);
    c->n_owners = n_owners;
    c->exp_rec.assign(h.begin(), h.begin() + n_owners);
    c->exp_heap.assign(h.begin() + n_owners, h.end());
    if (h_rec) memcpy(h_rec, c->exp_rec.data(), 8ull * n_owners);
    if (h_heap) memcpy(h_heap, c->exp_heap.data(), 8ull * n_owners);
}

// wait = false: the caller consumes the packed records on the context's stream (the library's own
// exchange): no host wait here
void export_pack(mrg_ctx *c, void *d_rec, void *d_heap, bool wait) {
    need_job(c);
    if (!c->n_owners) raise(MRG_EINVAL, "call mrg_job_export_sizes first");
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint32_t G = c->n_owners;
    std::vector<uint64_t> base(2ull * G, 0);
    for (uint32_t o = 1; o < G; ++o) {
        base[o] = base[o - 1] + c->exp_rec[o - 1];
        base[G + o] = base[G + o - 1] + c->exp_heap[o - 1];
    }
    uint64_t *d_base = sc.get<uint64_t>(2ull * G);
    unsigned long long *cur = sc.get<unsigned long long>(2ull * G);
    HIPCHK(hipMemcpyAsync(d_base, base.data(), 16ull * G, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(cur, 0, 16ull * G, s));
    mrg_launch_export_pack(c->keys.ks, c->keys.heap, c->keys.n, G, d_base, d_base + G, cur, cur + G, (XRec *)d_rec,
                           (uint8_t *)d_heap, is_idx(c), c->xrec_vmax, s);
    if (wait) sync(c);
}

// Received records -> the job's keys: exchange records (xr, include/mrgpu.h) or the text reduce's
// line records (lr, k_text.hip).
void import_recs(mrg_ctx *c, const XRec *xr, const LRec *lr, uint64_t n_rec, const void *d_heap, uint64_t heap_bytes,
                 const uint64_t *seg_recs, const uint64_t *seg_heap, uint32_t n_segs) {
    need_job(c);
    c->wide.release(c->pool);  // the imported records replace the job's keys, whatever path the map took
    acc_release(c);            // (and the accumulator of mrg_job_map_add)
    c->keyed = false;
    c->st.map_batches = 0;
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    std::vector<uint64_t> rec_end, heap_base;
    if (n_segs == 0) {
        rec_end.push_back(n_rec);
        heap_base.push_back(0);
        n_segs = 1;
    } else {
        uint64_t r = 0, h = 0;
        for (uint32_t i = 0; i < n_segs; ++i) {
            heap_base.push_back(h);
            r += seg_recs[i];
            h += seg_heap[i];
            rec_end.push_back(r);
        }
        if (r != n_rec || h != heap_bytes) raise(MRG_EINVAL, "segment sizes do not add up to n_rec / heap_bytes");
    }
    uint64_t *d_seg = sc.get<uint64_t>(2ull * n_segs);
    HIPCHK(hipMemcpyAsync(d_seg, rec_end.data(), 8ull * n_segs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_seg + n_segs, heap_base.data(), 8ull * n_segs, hipMemcpyHostToDevice, s));
    LongItems li{};
    li.base = (const uint8_t *)d_heap;
    li.start = sc.get<uint64_t>(n_rec);
    li.rawlen = sc.get<uint32_t>(n_rec);
    li.doc = sc.get<uint32_t>(n_rec);
    li.cnt = sc.get<uint64_t>(n_rec);
    li.verbatim = 1;  // the exchange heap holds exact key bytes
    HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_LONG], 0, 8, s));
    if (xr) mrg_launch_x_split_long(xr, n_rec, d_seg, d_seg + n_segs, n_segs, li, &c->d_cnt[CNT_LONG], is_idx(c), s);
    else mrg_launch_l_split_long(lr, n_rec, d_seg, d_seg + n_segs, n_segs, li, &c->d_cnt[CNT_LONG], s);
    read_counters(c);
    li.n = c->h_cnt[CNT_LONG];
    ShortSrc src;
    src.x = xr;
    src.lx = lr;
    src.n = n_rec;
    ev_rec(c, c->ev, 2);
    aggregate(c, src, li);
    ev_rec(c, c->ev, 3);
    sync(c);
    c->st.ms_aggregate = ev_ms(c, c->ev, 2, 3);
    c->mapped = c->keyed = true;
    c->reduced = false;
}

void job_import(mrg_ctx *c, const void *d_rec, uint64_t n_rec, const void *d_heap, uint64_t heap_bytes,
                const uint64_t *seg_recs, const uint64_t *seg_heap, uint32_t n_segs) {
    import_recs(c, (const XRec *)d_rec, nullptr, n_rec, d_heap, heap_bytes, seg_recs, seg_heap, n_segs);
}

// Test knob: MRG_TEST_FAIL="<stage>[:<rank>]" raises an injected failure at that stage (on that rank
// only, or on every rank), so the failure paths of the multi-GPU plan can be exercised.
void test_fail(const char *stage, int rank) {
    const char *v = getenv("MRG_TEST_FAIL");
    if (!v || !*v) return;
    const char *colon = strchr(v, ':');
    const size_t n = colon ? (size_t)(colon - v) : strlen(v);
    if (n == strlen(stage) && !strncmp(v, stage, n) && (!colon || atoi(colon + 1) == rank))
        raise(MRG_EINVAL, "injected failure at stage '%s' on rank %d (MRG_TEST_FAIL)", stage, rank);
}

// Abort from any thread (mrg_run_job's watchdog), serialised with the rank threads' enqueues until
// `deadline`.  An enqueue can itself block inside RCCL (a first send/recv to a peer sets up the
// connection and waits for that peer): a lock still held at the deadline belongs to such a blocked
// call, and the abort then goes ahead without the lock -- the accepted exception to the lock's rule,
// since releasing a blocked call is exactly what ncclCommAbort exists for.  The watchdog aborts all
// ranks in parallel against one deadline (a job with G hung ranks waits once, not G times).
void comm_abort(mrg_comm *m, std::chrono::steady_clock::time_point deadline) {
    std::unique_lock<std::timed_mutex> lk(m->mu, std::defer_lock);
    (void)lk.try_lock_until(deadline);
    if (m->comm && !m->aborted.exchange(true)) (void)ncclCommAbort(m->comm);
}

// The communicators of one mrg_run_job, rank g on devices[g]: all of them in one call (nothing to wait for
// if one cannot be made).  On a failure none is left: those not yet handed to a mrg_comm are destroyed here,
// the ranks already made as mrg_comm_destroy does.
std::vector<mrg_comm *> comm_init_all(const std::vector<int> &devices) {
    const int G = (int)devices.size();
    std::vector<mrg_comm *> ms(G, nullptr);
    std::vector<ncclComm_t> cs(G, nullptr);
    const ncclResult_t r = ncclCommInitAll(cs.data(), G, devices.data());
    if (r != ncclSuccess) raise(MRG_ECOMM, "ncclCommInitAll over %d GPUs: %s", G, ncclGetErrorString(r));
    for (int g = 0; g < G; ++g) {
        try {
            ms[g] = comm_alloc(devices[g], G, g);
        } catch (...) {
            for (int k = g; k < G; ++k) { (void)hipSetDevice(devices[k]); (void)ncclCommDestroy(cs[k]); }
            for (int k = 0; k < g; ++k) (void)mrg_comm_destroy(ms[k]);
            throw;
        }
        ms[g]->comm = cs[g];
    }
    return ms;
}

// The shuffle: the reference's map -> reduce hand-off through mr-{m}-{r}.txt files
// (worker.rs:117-140 -> 79-109) as one exchange over RCCL.  Owner of partition r = r % G.
//
// Failure protocol: every rank reaches every collective of the exchange.  A rank whose local step
// fails (export, buffer allocation) still takes part, with a failure status: the per-destination
// counts message carries it (the first collective), and one status all-reduce precedes the data
// transfer; every rank then raises together (the failing rank its own error, the others MRG_ECOMM).
// An RCCL error aborts the communicator.

void job_shuffle(mrg_ctx *c, mrg_comm *m) {
    if (!c || !m || !m->comm) raise(MRG_EINVAL, "null context or communicator");
    if (m->device != c->device) raise(MRG_EINVAL, "communicator is on device %d, context on %d", m->device, c->device);
    check_not_aborted(m);
    hipStream_t s = c->stream;
    const uint32_t G = (uint32_t)m->n;
    const uint32_t me = (uint32_t)m->rank;
    const uint64_t X = MRG_XREC_BYTES;
    // send records / heap, receive records / heap: returned on every exit (a failed collective or a
    // watchdog abort throws past the success path)
    Scratch buf(c->pool);
    uint8_t *srec = nullptr, *sheap = nullptr, *rrec = nullptr, *rheap = nullptr;
    MrgError mine{MRG_OK, ""};
    // ---- local: export sizes and pack (the pack runs on the stream, no host wait)
    std::vector<uint64_t> sc(3ull * G, 0), rc(3ull * G, 0);  // per peer: records, heap bytes, status
    std::vector<uint64_t> sro(G + 1, 0), sho(G + 1, 0);
    try {
        need_job(c);
        if (!c->mapped) raise(MRG_EINVAL, "shuffle before map");
        test_fail("export", (int)me);
        export_sizes(c, G, nullptr, nullptr);
        for (uint32_t o = 0; o < G; ++o) {
            sc[3 * o] = c->exp_rec[o];
            sc[3 * o + 1] = c->exp_heap[o];
            sro[o + 1] = sro[o] + sc[3 * o];
            sho[o + 1] = sho[o] + sc[3 * o + 1];
        }
        srec = buf.get<uint8_t>(sro[G] * X + 16);
        sheap = buf.get<uint8_t>(sho[G] + 16);
        export_pack(c, srec, sheap, false);
    } catch (const MrgError &e) {
        mine = e;
        std::fill(sc.begin(), sc.end(), 0);
    }
    for (uint32_t o = 0; o < G; ++o) sc[3 * o + 2] = mine.code ? 1u : 0u;
    // ---- collective 1: the counts all-to-all (with every rank's status)
    HIPCHK(hipMemcpyAsync(m->d_counts, sc.data(), 24ull * G, hipMemcpyHostToDevice, s));
    {
        CommLock lk(m);
        nccl_or_abort(m, ncclAllToAll(m->d_counts, m->d_counts + 3 * G, 3, ncclUint64, m->comm, s), "ncclAllToAll");
    }
    HIPCHK(hipMemcpyAsync(rc.data(), m->d_counts + 3 * G, 24ull * G, hipMemcpyDeviceToHost, s));
    sync(c);
    check_not_aborted(m);
    int failed_peer = -1;
    for (uint32_t o = 0; o < G; ++o)
        if (rc[3 * o + 2] && failed_peer < 0) failed_peer = (int)o;
    if (mine.code) throw mine;
    if (failed_peer >= 0) raise(MRG_ECOMM, "rank %d of the exchange failed before sending", failed_peer);
    // ---- local: receive buffers
    std::vector<uint64_t> rro(G + 1, 0), rho(G + 1, 0), seg_rec(G), seg_heap(G);
    for (uint32_t o = 0; o < G; ++o) {
        rro[o + 1] = rro[o] + rc[3 * o];
        rho[o + 1] = rho[o] + rc[3 * o + 1];
        seg_rec[o] = rc[3 * o];
        seg_heap[o] = rc[3 * o + 1];
    }
    try {
        test_fail("recv", (int)me);
        rrec = buf.get<uint8_t>(rro[G] * X + 16);
        rheap = buf.get<uint8_t>(rho[G] + 16);
    } catch (const MrgError &e) {
        mine = e;
    }
    // ---- collective 2: everyone ready to transfer?
    if (agree(c, m, mine.code ? 1 : 0)) {
        if (mine.code) throw mine;
        raise(MRG_ECOMM, "another rank of the exchange could not allocate its receive buffers");
    }
    // ---- collective 3: own slice by a device copy; peers by one send/recv group (each peer pair has
    // its own xGMI link)
    EventPair ev;
    HIPCHK(hipEventRecord(ev.e0, s));
    if (sc[3 * me]) HIPCHK(hipMemcpyAsync(rrec + rro[me] * X, srec + sro[me] * X, sc[3 * me] * X, hipMemcpyDeviceToDevice, s));
    if (sc[3 * me + 1]) HIPCHK(hipMemcpyAsync(rheap + rho[me], sheap + sho[me], sc[3 * me + 1], hipMemcpyDeviceToDevice, s));
    uint64_t sent = 0, recv = 0;
    {
        CommLock lk(m);
        nccl_or_abort(m, ncclGroupStart(), "ncclGroupStart");
        // test knob: an RCCL failure inside the group, after the events and all four buffers exist
        if (getenv("MRG_TEST_FAIL")) {
            try {
                test_fail("sendrecv", (int)me);
            } catch (const MrgError &) {
                group_or_abort(m, ncclInternalError, "ncclSend (MRG_TEST_FAIL=sendrecv)");
            }
        }
        for (uint32_t o = 0; o < G; ++o) {
            if (o == me) continue;
            if (sc[3 * o]) group_or_abort(m, ncclSend(srec + sro[o] * X, sc[3 * o] * X, ncclUint8, (int)o, m->comm, s), "ncclSend");
            if (sc[3 * o + 1]) group_or_abort(m, ncclSend(sheap + sho[o], sc[3 * o + 1], ncclUint8, (int)o, m->comm, s), "ncclSend");
            if (rc[3 * o]) group_or_abort(m, ncclRecv(rrec + rro[o] * X, rc[3 * o] * X, ncclUint8, (int)o, m->comm, s), "ncclRecv");
            if (rc[3 * o + 1]) group_or_abort(m, ncclRecv(rheap + rho[o], rc[3 * o + 1], ncclUint8, (int)o, m->comm, s), "ncclRecv");
            sent += sc[3 * o] * X + sc[3 * o + 1];
            recv += rc[3 * o] * X + rc[3 * o + 1];
        }
        nccl_or_abort(m, ncclGroupEnd(), "ncclGroupEnd");
    }
    HIPCHK(hipEventRecord(ev.e1, s));
    HIPCHK(hipEventSynchronize(ev.e1));
    check_not_aborted(m);  // a watchdog abort ends a transfer early: its buffers are not to be used
    buf.put(srec);
    buf.put(sheap);
    // ---- local: re-aggregate what arrived (no collective after this point)
    const mrg_stats keep = c->st;
    job_import(c, rrec, rro[G], rheap, rho[G], seg_rec.data(), seg_heap.data(), G);  // ends with a host wait
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    // the import's aggregation time is the reduce side's; the map-side stats stay those of the map
    const double agg_import = c->st.ms_aggregate;
    c->st = keep;
    c->st.ms_aggregate += agg_import;
    c->st.distinct_keys = c->keys.n;
    c->st.ms_exchange = ms;
    c->st.exchange_sent = sent;
    c->st.exchange_recv = recv;
}

}  // namespace mrg_host

extern "C" {

int mrg_comm_get_id(uint8_t id[MRG_COMM_ID_BYTES]) {
    return guard([&] {
        if (!id) raise(MRG_EINVAL, "null id");
        static_assert(sizeof(ncclUniqueId) == MRG_COMM_ID_BYTES, "RCCL unique id size");
        ncclUniqueId u;
        NCCLCHK(ncclGetUniqueId(&u));
        memcpy(id, &u, sizeof u);
    });
}

int mrg_comm_init(mrg_ctx *c, const uint8_t id[MRG_COMM_ID_BYTES], int n_ranks, int rank, mrg_comm **out) {
    return guard([&] {
        if (!c || !id || !out) raise(MRG_EINVAL, "null argument");
        if (n_ranks < 1 || rank < 0 || rank >= n_ranks) raise(MRG_EINVAL, "rank %d of %d", rank, n_ranks);
        HIPCHK(hipSetDevice(c->device));
        ncclUniqueId u;
        memcpy(&u, id, sizeof u);
        // the buffers first: a rank that fails here has not joined, and its peers' init fails or
        // waits for it (the caller's concern: mrg_run_job creates its communicators in one call)
        mrg_comm *m = comm_alloc(c->device, n_ranks, rank);
        const ncclResult_t r = ncclCommInitRank(&m->comm, n_ranks, u, rank);
        if (r != ncclSuccess) {
            comm_free(m);
            raise(MRG_ECOMM, "ncclCommInitRank(%d of %d): %s", rank, n_ranks, ncclGetErrorString(r));
        }
        *out = m;
    });
}

int mrg_comm_destroy(mrg_comm *m) {
    return guard([&] {
        if (!m) return;
        ncclResult_t r = ncclSuccess;
        if (m->comm && !m->aborted.load()) {
            (void)hipSetDevice(m->device);
            r = ncclCommDestroy(m->comm);
        }
        m->comm = nullptr;
        comm_free(m);
        if (r != ncclSuccess) raise(MRG_ECOMM, "ncclCommDestroy: %s", ncclGetErrorString(r));
    });
}

int mrg_job_shuffle(mrg_ctx *c, mrg_comm *m) {
    return guard([&] { job_shuffle(c, m); });
}

int mrg_comm_count(const mrg_comm *m, int *n_ranks) {
    return guard([&] {
        if (!m || !n_ranks) raise(MRG_EINVAL, "null argument");
        if (!m->comm || m->aborted.load()) raise(MRG_ECOMM, "the communicator was aborted");
        int n = 0;
        const ncclResult_t r = ncclCommCount(m->comm, &n);
        if (r != ncclSuccess) raise(MRG_ECOMM, "ncclCommCount: %s", ncclGetErrorString(r));
        *n_ranks = n;
    });
}

}  // extern "C"
