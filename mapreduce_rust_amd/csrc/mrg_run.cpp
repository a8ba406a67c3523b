// mrg_run.cpp -- mrg_run_job (include/mrgpu.h): a whole job from files to files on one or more GPUs -- the batch
// plan of MRG_FLAG_STREAM, the threaded file readers with their pinned staging, one host thread per rank with the
// watchdog that aborts the communicators of a failed exchange, the host merges of the ranks' final.txt and top.txt,
// the run statistics -- and the test entries that reach its host-only parts without a GPU (mrg_test_stream_plan,
// mrg_test_merge_sorted_lines, mrg_test_merge_top_lines).
// Calls: mrgpu.cpp (mrg_open, mrg_close, job_begin), mrg_map.cpp (job_map), mrg_agg.cpp (job_map_add),
// mrg_exchange.cpp (comm_init_all, comm_abort, job_shuffle, test_fail, mrg_comm_destroy), mrg_reduce.cpp
// (job_reduce, job_final, job_topk), mrg_plugin.cpp (check_names).  Nothing calls into it but the C ABI.
#include <sys/stat.h>

#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <thread>

#include "mrg_comm.h"

using namespace mrg_host;

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

thread_local mrg_run_stats g_run{};
thread_local uint32_t g_stream_batches = 0;   // mrg_run_get_stream_stats
thread_local uint64_t g_stream_peak = 0;

// MRG_FLAG_STREAM: the batches of one GPU's files, first[i] = first file of batch i.  A batch is a
// maximal run of consecutive files whose sizes sum to at most batch_bytes; a larger file is a batch of
// its own; zero-length files join their neighbours (they never end a run that still has room).
std::vector<uint32_t> stream_plan(const uint64_t *sizes, size_t n, uint64_t batch_bytes) {
    std::vector<uint32_t> first;
    for (size_t i = 0; i < n;) {
        first.push_back((uint32_t)i);
        uint64_t sum = sizes[i++];
        while (i < n && sum <= batch_bytes && sizes[i] <= batch_bytes - sum) sum += sizes[i++];
    }
    return first;
}

void write_file(const std::string &path, const uint8_t *p, uint64_t n) {
    FILE *f = fopen(path.c_str(), "wb");  // worker.rs:167-168 File::create("mr-{r}.txt")
    if (!f) raise(MRG_EIO, "cannot create %s", path.c_str());
    const size_t w = n ? fwrite(p, 1, n, f) : 0;
    const int cl = fclose(f);
    if (w != n || cl != 0) raise(MRG_EIO, "short write on %s", path.c_str());
}

// k-way merge of G byte-sorted line runs (each GPU's final.txt lines): LC_ALL=C `sort` order.  A run
// may lack its final newline (its last line then ends at the run's end); each cursor's line end is
// found once per line.
std::vector<uint8_t> merge_sorted_lines(const std::vector<std::pair<const uint8_t *, uint64_t>> &runs) {
    struct Cur { const uint8_t *p, *e, *le; };  // le = end of the current line (its '\n' or e)
    std::vector<Cur> cur;
    uint64_t total = 0;
    auto line_end = [](const uint8_t *p, const uint8_t *e) {
        const uint8_t *q = (const uint8_t *)memchr(p, '\n', (size_t)(e - p));
        return q ? q : e;
    };
    for (auto &r : runs) {
        if (!r.second) continue;
        cur.push_back({r.first, r.first + r.second, line_end(r.first, r.first + r.second)});
        total += r.second;
    }
    std::vector<uint8_t> out;
    out.reserve(total + runs.size());
    while (!cur.empty()) {
        size_t best = 0;
        for (size_t i = 1; i < cur.size(); ++i) {
            const size_t la = (size_t)(cur[i].le - cur[i].p), lb = (size_t)(cur[best].le - cur[best].p);
            const int cm = memcmp(cur[i].p, cur[best].p, std::min(la, lb));
            if (cm < 0 || (cm == 0 && la < lb)) best = i;
        }
        Cur &c = cur[best];
        out.insert(out.end(), c.p, c.le);
        out.push_back('\n');  // every output line ends with a newline, also a run's unterminated last one
        c.p = c.le < c.e ? c.le + 1 : c.e;
        if (c.p >= c.e) cur.erase(cur.begin() + (ptrdiff_t)best);
        else c.le = line_end(c.p, c.e);
    }
    return out;
}

// k-way merge of G runs of "key count" lines, each ordered by (count descending, key bytes ascending)
// -- each GPU's mrg_job_topk lines -- keeping the first k lines.  The count is the digits after the
// line's last space, compared as a decimal string (no leading zeros: longer is larger), so any number
// of digits works.  A run may be empty or lack its final newline.
std::vector<uint8_t> merge_top_lines(const std::vector<std::pair<const uint8_t *, uint64_t>> &runs, uint64_t k) {
    struct Cur { const uint8_t *p, *e, *le, *sp; };  // le = end of the current line, sp = its last space (or le)
    auto line_end = [](const uint8_t *p, const uint8_t *e) {
        const uint8_t *q = (const uint8_t *)memchr(p, '\n', (size_t)(e - p));
        return q ? q : e;
    };
    auto last_space = [](const uint8_t *p, const uint8_t *le) {
        const uint8_t *q = (const uint8_t *)memrchr(p, ' ', (size_t)(le - p));
        return q ? q : le;
    };
    // a before b
    auto before = [](const Cur &a, const Cur &b) {
        const size_t da = a.sp < a.le ? (size_t)(a.le - a.sp - 1) : 0, db = b.sp < b.le ? (size_t)(b.le - b.sp - 1) : 0;
        if (da != db) return da > db;
        const int cc = da ? memcmp(a.sp + 1, b.sp + 1, da) : 0;
        if (cc) return cc > 0;
        const size_t ka = (size_t)(a.sp - a.p), kb = (size_t)(b.sp - b.p);
        const int cm = memcmp(a.p, b.p, std::min(ka, kb));
        return cm < 0 || (cm == 0 && ka < kb);
    };
    std::vector<Cur> cur;
    for (auto &r : runs) {
        if (!r.second) continue;
        const uint8_t *e = r.first + r.second, *le = line_end(r.first, e);
        cur.push_back({r.first, e, le, last_space(r.first, le)});
    }
    std::vector<uint8_t> out;
    for (uint64_t taken = 0; taken < k && !cur.empty(); ++taken) {
        size_t best = 0;
        for (size_t i = 1; i < cur.size(); ++i)
            if (before(cur[i], cur[best])) best = i;
        Cur &c = cur[best];
        out.insert(out.end(), c.p, c.le);
        out.push_back('\n');
        c.p = c.le < c.e ? c.le + 1 : c.e;
        if (c.p >= c.e) {
            cur.erase(cur.begin() + (ptrdiff_t)best);
        } else {
            c.le = line_end(c.p, c.e);
            c.sp = last_space(c.p, c.le);
        }
    }
    return out;
}

// ---- input files -> device: worker.rs:65-77 reads each file whole (read_to_string).  Here the
// files of a GPU are read in chunks by several host threads into pinned staging buffers (two per
// thread), each chunk copied to the device buffer while the thread reads the next one, so disk /
// page-cache reads and the PCIe copies overlap.
struct FileChunk {
    uint32_t file;   // index in the rank's file list
    uint64_t off, n; // bytes [off, off + n) of the file
    uint64_t dst;    // offset in the device buffer
};

constexpr uint64_t MRG_READ_CHUNK = 32ull << 20;
// MRG_FLAG_STREAM reads with smaller chunks: the readers' pinned staging (two chunks per thread) is made
// and freed once per job, at a cost that grows with its size and that no longer hides in a long read
// (measured: DESIGN.md section 18)
constexpr uint64_t MRG_STREAM_READ_CHUNK = 8ull << 20;

// The reader threads' pinned staging buffers, copy streams and events.  One call makes and frees its
// own; a caller that reads batch after batch (MRG_FLAG_STREAM) keeps one across its calls -- pinning
// the buffers again for every batch cost more than reading it.
struct ReadStage {
    struct Slot {
        hipStream_t st = nullptr;
        uint8_t *pin[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        uint64_t bytes = 0;
        void release() {
            if (st) (void)hipStreamSynchronize(st);
            for (int k = 0; k < 2; ++k) {
                if (ev[k]) (void)hipEventDestroy(ev[k]);
                if (pin[k]) (void)hipHostFree(pin[k]);
            }
            if (st) (void)hipStreamDestroy(st);
            *this = Slot{};
        }
    };
    int device = 0;
    std::vector<Slot> slots;  // one per reader thread
    ~ReadStage() {
        (void)hipSetDevice(device);
        for (auto &sl : slots) sl.release();
    }
};

void read_files_to_device(int device, const std::vector<const char *> &paths, const std::vector<uint64_t> &doc_off,
                          uint8_t *d, int n_threads, ReadStage *stage = nullptr, uint64_t chunk_dflt = MRG_READ_CHUNK) {
    std::vector<FileChunk> chunks;
    // (MRG_READ_CHUNK_MIB: a tuning knob for the staging size, tools/time_stream.py)
    const uint64_t chunk = std::max<uint64_t>(1, env_u64("MRG_READ_CHUNK_MIB", chunk_dflt >> 20)) << 20;
    for (uint32_t i = 0; i < paths.size(); ++i) {
        const uint64_t sz = doc_off[i + 1] - doc_off[i];
        for (uint64_t o = 0; o < sz; o += chunk)
            chunks.push_back({i, o, std::min<uint64_t>(chunk, sz - o), doc_off[i] + o});
    }
    if (chunks.empty()) return;
    n_threads = std::max(1, std::min<int>(n_threads, (int)chunks.size()));
    uint64_t pin_bytes = 0;  // staging buffers sized to the largest chunk (small inputs: small buffers)
    for (auto &ch : chunks) pin_bytes = std::max(pin_bytes, ch.n);
    std::atomic<size_t> next{0};
    std::atomic<int> fail{0};
    std::vector<int> rc(n_threads, MRG_OK);
    std::vector<std::string> msg(n_threads);
    if (stage) {
        stage->device = device;
        if (stage->slots.size() < (size_t)n_threads) stage->slots.resize((size_t)n_threads);
    }
    auto reader = [&](int t) {
        rc[t] = guard([&] {
            HIPCHK(hipSetDevice(device));
            ReadStage::Slot local;
            ReadStage::Slot &sl = stage ? stage->slots[(size_t)t] : local;
            std::vector<int> fds(paths.size(), -1);
            struct Res {  // on every exit path: the copies done, the files closed, a one-call stage freed
                ReadStage::Slot &sl; bool own; std::vector<int> &fds;
                ~Res() {
                    if (sl.st) (void)hipStreamSynchronize(sl.st);
                    if (own) sl.release();
                    for (int fd : fds) if (fd >= 0) close(fd);
                }
            } res{sl, stage == nullptr, fds};
            if (sl.bytes < pin_bytes) {  // (a kept stage grows to the largest chunk it meets)
                sl.release();
                HIPCHK(hipStreamCreateWithFlags(&sl.st, hipStreamNonBlocking));
                for (int k = 0; k < 2; ++k) {
                    HIPCHK(hipHostMalloc(&sl.pin[k], pin_bytes, hipHostMallocDefault));
                    HIPCHK(hipEventCreateWithFlags(&sl.ev[k], hipEventDisableTiming));
                }
                sl.bytes = pin_bytes;
            }
            hipStream_t st = sl.st;
            uint8_t **pin = sl.pin;
            hipEvent_t *ev = sl.ev;
            bool used[2] = {false, false};
            for (int k = 0;; k ^= 1) {
                if (fail.load()) return;
                const size_t ci = next.fetch_add(1);
                if (ci >= chunks.size()) break;
                const FileChunk &ch = chunks[ci];
                if (used[k]) HIPCHK(hipEventSynchronize(ev[k]));  // the copy out of this buffer is done
                int &fd = fds[ch.file];
                if (fd < 0) {
                    fd = open(paths[ch.file], O_RDONLY);  // worker.rs:73 File::open(..).unwrap()
                    if (fd < 0) raise(MRG_EIO, "cannot open %s", paths[ch.file]);
                }
                uint64_t got = 0;
                while (got < ch.n) {
                    const ssize_t r = pread(fd, pin[k] + got, (size_t)(ch.n - got), (off_t)(ch.off + got));
                    if (r <= 0) raise(MRG_EIO, "short read on %s", paths[ch.file]);
                    got += (uint64_t)r;
                }
                HIPCHK(hipMemcpyAsync(d + ch.dst, pin[k], ch.n, hipMemcpyHostToDevice, st));
                HIPCHK(hipEventRecord(ev[k], st));
                used[k] = true;
            }
            HIPCHK(hipStreamSynchronize(st));
        });
        if (rc[t]) {
            msg[t] = g_err;
            fail.store(1);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < n_threads; ++t) th.emplace_back(reader, t);
    reader(0);
    for (auto &x : th) x.join();
    for (int t = 0; t < n_threads; ++t)
        if (rc[t]) raise(rc[t], "%s", msg[t].c_str());
}

// One GPU of mrg_run_job.
struct RankState {
    int g = 0, device = 0;
    mrg_ctx *c = nullptr;
    mrg_comm *m = nullptr;
    uint8_t *d = nullptr, *d2 = nullptr;  // device input (MRG_FLAG_STREAM: the two batch buffers)
    uint64_t in_bytes = 0, buf_bytes = 0;
    uint32_t batches = 0;
    std::vector<uint8_t> out, fin, top;
};

// Runs fn on every rank, one host thread each, and returns when all have returned; the per-rank
// status codes and messages are left in rc / msg.  In a phase with collectives (`watch`), a rank
// that failed outside the exchange's own status protocol (an RCCL error) can leave its peers
// waiting for it: once a rank has failed and the others have not finished within the grace period
// (MRG_ABORT_GRACE_MS, default 10 s), every communicator is aborted, so the waiting RCCL operations
// fail and their threads return.
template <class F>
void run_ranks(std::vector<RankState> &rs, bool watch, F &&fn, std::vector<int> &rc, std::vector<std::string> &msg) {
    const int G = (int)rs.size();
    rc.assign(G, MRG_OK);
    msg.assign(G, std::string());
    std::mutex mu;
    std::condition_variable cv;
    int done = 0, failed = 0;
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g)
        th.emplace_back([&, g] {
            const int r = guard([&] {
                HIPCHK(hipSetDevice(rs[g].device));
                fn(rs[g]);
            });
            std::lock_guard<std::mutex> lk(mu);
            rc[g] = r;
            if (r) {
                msg[g] = g_err;
                ++failed;
            }
            ++done;
            cv.notify_all();
        });
    const uint64_t grace_ms = env_u64("MRG_ABORT_GRACE_MS", 10000);
    {
        std::unique_lock<std::mutex> lk(mu);
        Clock::time_point first_fail{};
        bool aborted = false;
        while (done < G) {
            cv.wait_for(lk, std::chrono::milliseconds(50));
            if (!watch || aborted || !failed || done >= G) continue;
            if (first_fail == Clock::time_point{}) first_fail = Clock::now();
            if (ms_since(first_fail) < (double)grace_ms) continue;
            aborted = true;
            lk.unlock();  // the rank threads report in while their communicators are aborted
            const auto deadline = Clock::now() + std::chrono::milliseconds(2000);
            std::vector<std::thread> ab;
            for (auto &r : rs)
                if (r.m) ab.emplace_back([m = r.m, deadline] { comm_abort(m, deadline); });
            for (auto &t : ab) t.join();
            lk.lock();
        }
    }
    for (auto &t : th) t.join();
}

// The first failure that is not an echo (MRG_ECOMM) of another rank's, else the first failure.
void raise_first(const std::vector<int> &rc, const std::vector<std::string> &msg, const std::vector<RankState> &rs) {
    for (size_t g = 0; g < rc.size(); ++g)
        if (rc[g] && rc[g] != MRG_ECOMM) raise(rc[g], "GPU %d: %s", rs[g].device, msg[g].c_str());
    for (size_t g = 0; g < rc.size(); ++g)
        if (rc[g]) raise(rc[g], "GPU %d: %s", rs[g].device, msg[g].c_str());
}

void release_ranks(std::vector<RankState> &rs) {
    for (auto &r : rs) {
        if (r.d && r.c) {
            (void)hipSetDevice(r.device);
            r.c->pool.put(r.d);
            r.c->pool.put(r.d2);
        }
        if (r.m) (void)mrg_comm_destroy(r.m);
        if (r.c) (void)mrg_close(r.c);
        r = RankState{};
    }
}

// The whole job on GPUs devices[0..G): the static plan for the coordinator's task assignment
// (coordinator.rs:137-215) and the workers' map-then-reduce loop (mrworker.rs:43-149).  Phases, each
// on all GPUs at once and joined before the next: open contexts -> create the communicators (one
// ncclCommInitAll) -> read + map -> exchange -> reduce + write.  A failure in any phase fails the job
// there: before the communicators exist nothing collective has started, and the exchange agrees on
// every rank's status before each of its transfers, so no GPU thread is left waiting for another.
void run_job(const char *const *files, size_t n_files, uint32_t R, int app, const char *out_dir, uint32_t flags,
             const std::vector<int> &devices) {
    const Clock::time_point t_all = Clock::now();
    g_run = mrg_run_stats{};
    g_stream_batches = 0;
    g_stream_peak = 0;
    const int G = (int)devices.size();
    g_run.n_gpus = G;
    const uint64_t top_k = flags >> 16;  // MRG_FLAG_TOP(k): also out_dir/top.txt
    std::vector<const char *> names(files, files + n_files);
    check_names(names.data(), (uint32_t)n_files);
    std::vector<RankState> rs(G);
    struct Guard { std::vector<RankState> &rs; ~Guard() { release_ranks(rs); } } release{rs};
    std::vector<int> rc;
    std::vector<std::string> msg;
    // ---- contexts (worker processes)
    Clock::time_point t0 = Clock::now();
    for (int g = 0; g < G; ++g) {
        rs[g].g = g;
        rs[g].device = devices[g];
        test_fail("open", g);
        if (mrg_open(devices[g], &rs[g].c) != MRG_OK) raise(MRG_EHIP, "GPU %d: %s", devices[g], mrg_last_error());
    }
    // ---- communicators: all of them in one call (nothing to wait for if one cannot be made)
    const bool comm = G > 1 || env_u64("MRG_TEST_FORCE_COMM", 0);
    if (comm) {
        test_fail("comm", 0);
        const std::vector<mrg_comm *> ms = comm_init_all(devices);
        for (int g = 0; g < G; ++g) rs[g].m = ms[g];
    }
    g_run.ms_open = ms_since(t0);
    // ---- map phase: GPU g reads and maps files m with m % G == g (coordinator.rs:137-176)
    const int readers = (int)std::max<uint64_t>(1, env_u64("MRG_READ_THREADS", std::max(1, std::min(16, 32 / G))));
    std::vector<double> t_read(G, 0.0), t_alloc(G, 0.0), t_mapk(G, 0.0), t_aggk(G, 0.0);
    t0 = Clock::now();
    run_ranks(rs, false, [&](RankState &r) {
        mrg_ctx *c = r.c;
        test_fail("map", r.g);
        const Clock::time_point tr = Clock::now();
        job_begin(c, app, R, flags);
        c->names.assign(files, files + n_files);
        std::vector<const char *> mine;
        std::vector<uint64_t> off(1, 0);
        std::vector<uint32_t> ids;
        for (size_t m = (size_t)r.g; m < n_files; m += (size_t)G) {
            struct stat sb;
            if (stat(files[m], &sb) != 0) raise(MRG_EIO, "cannot open %s", files[m]);  // worker.rs:73
            mine.push_back(files[m]);
            off.push_back(off.back() + (uint64_t)sb.st_size);
            ids.push_back((uint32_t)m);
        }
        r.in_bytes = off.back();
        double a0 = 0.0, a1 = 0.0;
        if (flags & MRG_FLAG_STREAM) {
            // batches of whole files, mapped one at a time (mrg_job_map_add) while a helper thread reads
            // the next one into the other buffer.  Both buffers are taken here: the pool is not
            // thread-safe, and the helper touches neither it nor the context.
            std::vector<uint64_t> sizes;
            for (size_t i = 0; i + 1 < off.size(); ++i) sizes.push_back(off[i + 1] - off[i]);
            uint64_t bb = env_u64("MRG_STREAM_BATCH_BYTES", 0);
            if (!bb) bb = 4ull << 30;  // the best of 256 MiB / 1 GiB / 4 GiB measured
            std::vector<uint32_t> first = stream_plan(sizes.data(), sizes.size(), bb);
            const size_t nb = first.size();
            first.push_back((uint32_t)sizes.size());
            uint64_t maxb = 0;
            for (size_t i = 0; i < nb; ++i) maxb = std::max(maxb, off[first[i + 1]] - off[first[i]]);
            uint8_t *buf[2] = {nullptr, nullptr};
            if (nb) buf[0] = r.d = pget<uint8_t>(c->pool, maxb + 64);
            if (nb > 1) buf[1] = r.d2 = pget<uint8_t>(c->pool, maxb + 64);
            r.buf_bytes = (uint64_t)std::min<size_t>(nb, 2) * (maxb + 64);
            r.batches = (uint32_t)nb;
            c->pool.alloc_stats(nullptr, nullptr, &a0);
            c->timing = true;
            ReadStage stage;  // the readers' pinned buffers, kept over the batches (freed after the last join)
            struct Read {  // one batch's read on the helper thread
                std::thread th;
                int rc = MRG_OK;
                std::string msg;
                std::vector<const char *> paths;
                std::vector<uint64_t> boff;
            } rd;
            struct Join { Read &rd; ~Join() { if (rd.th.joinable()) rd.th.join(); } } join{rd};  // on every path
            auto start_read = [&](size_t i) {
                rd.rc = MRG_OK;
                rd.paths.assign(mine.begin() + first[i], mine.begin() + first[i + 1]);
                rd.boff.assign(1, 0);
                for (uint32_t f = first[i]; f < first[i + 1]; ++f) rd.boff.push_back(off[f + 1] - off[first[i]]);
                uint8_t *dst = buf[i & 1];
                rd.th = std::thread([&rd, &stage, dst, dev = c->device, readers] {
                    rd.rc = guard([&] {
                        HIPCHK(hipSetDevice(dev));
                        read_files_to_device(dev, rd.paths, rd.boff, dst, readers, &stage, MRG_STREAM_READ_CHUNK);
                    });
                    if (rd.rc) rd.msg = g_err;
                });
            };
            double waited = ms_since(tr);  // (stat + plan + buffers: before the first read)
            double t_add = 0.0, t_start = 0.0;
            if (nb) start_read(0);
            for (size_t i = 0; i < nb; ++i) {
                const Clock::time_point tw = Clock::now();
                rd.th.join();
                waited += ms_since(tw);
                if (rd.rc) raise(rd.rc, "%s", rd.msg.c_str());
                const std::vector<uint64_t> boff = rd.boff;
                // buffer (i + 1) & 1 is free: the map of batch i - 1 has returned (it waits for the stream)
                const Clock::time_point ts = Clock::now();
                if (i + 1 < nb) start_read(i + 1);
                t_start += ms_since(ts);
                c->d_in = buf[i & 1];
                c->doc_off = boff;
                c->doc_ids.assign(ids.begin() + first[i], ids.begin() + first[i + 1]);
                const Clock::time_point ta = Clock::now();
                job_map_add(c);
                t_add += ms_since(ta);
                t_mapk[r.g] += c->st.ms_map;
                t_aggk[r.g] += c->st.ms_aggregate;
            }
            if (!nb) {  // no files: an empty job, as the unstreamed path maps an empty input
                r.d = pget<uint8_t>(c->pool, 64);
                c->d_in = r.d;
                c->doc_off.assign(1, 0);
                c->doc_ids.clear();
                job_map_add(c);
            }
            t_read[r.g] = waited;
            c->pool.alloc_stats(nullptr, nullptr, &a1);
            t_alloc[r.g] = a1 - a0;
            if (getenv("MRG_DEBUG"))
                fprintf(stderr, "[mrgpu] stream GPU %d: %zu batches, waited for reads %.2f ms, map_add calls %.2f ms, "
                        "read starts %.2f ms, phase so far %.2f ms\n", r.g, nb, waited, t_add, t_start, ms_since(tr));
            return;
        }
        r.buf_bytes = off.back();
        r.d = pget<uint8_t>(c->pool, off.back() + 64);
        read_files_to_device(c->device, mine, off, r.d, readers);
        t_read[r.g] = ms_since(tr);
        c->d_in = r.d;
        c->doc_off = off;
        c->doc_ids = ids;
        c->pool.alloc_stats(nullptr, nullptr, &a0);
        c->timing = true;  // HIP events around the map and aggregation kernels (mrg_run_stats)
        job_map(c);
        c->pool.alloc_stats(nullptr, nullptr, &a1);
        t_alloc[r.g] = a1 - a0;
        t_mapk[r.g] = c->st.ms_map;
        t_aggk[r.g] = c->st.ms_aggregate;
    }, rc, msg);
    raise_first(rc, msg, rs);
    g_run.ms_map = ms_since(t0);
    for (int g = 0; g < G; ++g) {
        g_run.ms_map_alloc = std::max(g_run.ms_map_alloc, t_alloc[g]);
        g_run.ms_map_kernel = std::max(g_run.ms_map_kernel, t_mapk[g]);
        g_run.ms_aggregate_kernel = std::max(g_run.ms_aggregate_kernel, t_aggk[g]);
        g_run.ms_read = std::max(g_run.ms_read, t_read[g]);
        g_run.input_bytes += rs[g].in_bytes;
        g_stream_batches = std::max(g_stream_batches, rs[g].batches);
        g_stream_peak = std::max(g_stream_peak, rs[g].buf_bytes);
    }
    g_run.ms_map -= g_run.ms_read;
    // ---- exchange (RCCL over xGMI)
    if (comm) {
        t0 = Clock::now();
        run_ranks(rs, true, [&](RankState &r) { job_shuffle(r.c, r.m); }, rc, msg);
        raise_first(rc, msg, rs);
        g_run.ms_shuffle = ms_since(t0);
    }
    // ---- reduce phase: GPU g formats the partitions r % G == g (coordinator.rs:178-215)
    t0 = Clock::now();
    run_ranks(rs, false, [&](RankState &r) {
        mrg_ctx *c = r.c;
        test_fail("reduce", r.g);
        job_reduce(c);
        r.out.resize(c->out_bytes);
        if (c->out_bytes) HIPCHK(hipMemcpyAsync(r.out.data(), c->d_out, c->out_bytes, hipMemcpyDeviceToHost, c->stream));
        if (flags & MRG_FLAG_FINAL_TXT) {  // run.sh:16-20 generate_output: this GPU's lines, sorted on the device
            job_final(c);
            r.fin.resize(c->final_bytes);
            if (c->final_bytes)
                HIPCHK(hipMemcpyAsync(r.fin.data(), c->d_final, c->final_bytes, hipMemcpyDeviceToHost, c->stream));
        }
        if (top_k) {  // this GPU's most frequent lines among the keys it owns
            job_topk(c, top_k);
            r.top.resize(c->top_bytes);
            if (c->top_bytes) HIPCHK(hipMemcpyAsync(r.top.data(), c->d_top, c->top_bytes, hipMemcpyDeviceToHost, c->stream));
        }
        sync(c);
    }, rc, msg);
    raise_first(rc, msg, rs);
    g_run.ms_reduce = ms_since(t0);
    // ---- writes: mr-{r}.txt by the GPU that owns r (worker.rs:167-179), then final.txt
    t0 = Clock::now();
    run_ranks(rs, false, [&](RankState &r) {
        test_fail("write", r.g);
        for (uint32_t p = (uint32_t)r.g; p < R; p += (uint32_t)G) {
            const uint64_t a = r.c->part_off[p], b = r.c->part_off[p + 1];
            write_file(std::string(out_dir) + "/mr-" + std::to_string(p) + ".txt", r.out.data() + a, b - a);
        }
    }, rc, msg);
    raise_first(rc, msg, rs);
    for (auto &r : rs) g_run.output_bytes += r.out.size();
    if (flags & MRG_FLAG_FINAL_TXT) {
        std::vector<std::pair<const uint8_t *, uint64_t>> runs;
        for (auto &r : rs) runs.push_back({r.fin.data(), r.fin.size()});
        if (G == 1) write_file(std::string(out_dir) + "/final.txt", rs[0].fin.data(), rs[0].fin.size());
        else {
            const std::vector<uint8_t> all = merge_sorted_lines(runs);
            write_file(std::string(out_dir) + "/final.txt", all.data(), all.size());
        }
    }
    if (top_k) {  // exact: after the shuffle every key, and every partition's dropped key, is on one GPU
        if (G == 1) write_file(std::string(out_dir) + "/top.txt", rs[0].top.data(), rs[0].top.size());
        else {
            std::vector<std::pair<const uint8_t *, uint64_t>> runs;
            for (auto &r : rs) runs.push_back({r.top.data(), r.top.size()});
            const std::vector<uint8_t> all = merge_top_lines(runs, top_k);
            write_file(std::string(out_dir) + "/top.txt", all.data(), all.size());
        }
    }
    g_run.ms_write = ms_since(t0);
    g_run.ms_total = ms_since(t_all);
}

}  // namespace

extern "C" {

int mrg_run_job(const char *const *files, size_t n_files, uint32_t n_reduce, int app, const char *out_dir,
                uint32_t flags, int n_gpus) {
    return guard([&] {
        if ((n_files && !files) || !out_dir) raise(MRG_EINVAL, "null argument");
        if (n_reduce == 0) raise(MRG_EINVAL, "n_reduce must be > 0");
        if ((flags >> 16) && app == MRG_APP_INDEXER) raise(MRG_EINVAL, "MRG_FLAG_TOP: word count only");
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (n_gpus < 1 || n_gpus > ndev) raise(MRG_EINVAL, "n_gpus %d: %d devices visible", n_gpus, ndev);
        std::vector<int> devs(n_gpus);
        for (int g = 0; g < n_gpus; ++g) devs[g] = g;
        run_job(files, n_files, n_reduce, app, out_dir, flags, devs);
    });
}

int mrg_run_get_stats(mrg_run_stats *out) {
    return guard([&] {
        if (!out) raise(MRG_EINVAL, "null argument");
        *out = g_run;
    });
}

int mrg_run_get_stream_stats(uint32_t *batches, uint64_t *peak_input_bytes) {
    if (batches) *batches = g_stream_batches;
    if (peak_input_bytes) *peak_input_bytes = g_stream_peak;
    return MRG_OK;
}

// Test entry (not in include/mrgpu.h): the batch plan of MRG_FLAG_STREAM over one GPU's file sizes,
// callable without a GPU.  first[i] (room for n entries) = first file of batch i; *n_batches = batches.
int mrg_test_stream_plan(const uint64_t *sizes, size_t n, uint64_t batch_bytes, uint32_t *first, size_t *n_batches) {
    return guard([&] {
        if (!n_batches || (n && (!sizes || !first))) raise(MRG_EINVAL, "null argument");
        if (n > 0xFFFFFFFFull) raise(MRG_EINVAL, "too many files");
        const std::vector<uint32_t> f = stream_plan(sizes, n, batch_bytes);
        if (!f.empty()) memcpy(first, f.data(), sizeof(uint32_t) * f.size());
        *n_batches = f.size();
    });
}

// Test entry (not in include/mrgpu.h): the k-way merge of sorted line runs that builds a multi-GPU
// final.txt, callable without a GPU.  *out (free with mrg_free) receives the merged bytes.
int mrg_test_merge_sorted_lines(const uint8_t *const *runs, const uint64_t *sizes, size_t k, uint8_t **out,
                                uint64_t *out_len) {
    return guard([&] {
        if (!out || !out_len || (k && (!runs || !sizes))) raise(MRG_EINVAL, "null argument");
        std::vector<std::pair<const uint8_t *, uint64_t>> v;
        for (size_t i = 0; i < k; ++i) v.push_back({runs[i], sizes[i]});
        const std::vector<uint8_t> m = merge_sorted_lines(v);
        uint8_t *o = (uint8_t *)malloc(m.size() + 1);
        if (!o) raise(MRG_ENOMEM, "host allocation failed");
        if (!m.empty()) memcpy(o, m.data(), m.size());
        *out = o;
        *out_len = m.size();
    });
}

// Test entry (not in include/mrgpu.h): the merge of per-GPU top-k line runs (count descending, key
// ascending) that builds a multi-GPU top.txt, callable without a GPU.  *out: free with mrg_free.
int mrg_test_merge_top_lines(const uint8_t *const *runs, const uint64_t *sizes, size_t n_runs, uint64_t k, uint8_t **out,
                             uint64_t *out_len) {
    return guard([&] {
        if (!out || !out_len || (n_runs && (!runs || !sizes))) raise(MRG_EINVAL, "null argument");
        std::vector<std::pair<const uint8_t *, uint64_t>> v;
        for (size_t i = 0; i < n_runs; ++i) v.push_back({runs[i], sizes[i]});
        const std::vector<uint8_t> m = merge_top_lines(v, k);
        uint8_t *o = (uint8_t *)malloc(m.size() + 1);
        if (!o) raise(MRG_ENOMEM, "host allocation failed");
        if (!m.empty()) memcpy(o, m.data(), m.size());
        *out = o;
        *out_len = m.size();
    });
}

}  // extern "C"
