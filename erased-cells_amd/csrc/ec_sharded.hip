// ec_sharded.hip — one process driving the n GPUs of a node (SURVEY §8b `ec_shard_*`, §8e).
//
// A raster is cut into contiguous row-blocks, shard i on device i of the group.  Each device has
//   * a launch thread bound to it for life (HIP's current device is per host thread, and a launch costs the
//     host ≈5 µs: eight devices served by one thread would serialise 40 µs of launches in front of kernels
//     that take ≈55 µs per 1/8 shard of a 16384² raster; eight threads issue them side by side),
//   * a non-blocking stream with its reduction scratch,
//   * a 64-byte device payload slot and a 64-byte pinned host slot (two words for min/max and counts, one ec_moments for stats),
//   * an RCCL communicator of the n-device clique (ncclCommInitAll) unless EC_GROUP_HOST_COMBINE.
//
// Element-wise entry points are FIRE-AND-FORGET (round 3): the calling thread checks the arguments, copies the
// per-shard pointers into one job per launch thread, posts the jobs and returns — it does not wait for the launch
// threads to have issued.  A launch thread that has just run a job polls its queue for a few tens of microseconds
// before it sleeps, so back-to-back sharded calls cost the caller a queue push per device and no futex wake
// (profiles/r03/group_fanout.md).  A failure inside a posted job (a launch error) is recorded in the group and
// returned by the next ec_shard_group_sync or reduction.  Rounds 1-2 blocked every call on a latch until all
// threads had issued (EC_GROUP_BLOCKING_ISSUE keeps that form for comparison).
//
// The reductions are synchronous and run in phases, so that a shard that fails cannot leave the others waiting in a
// collective: (0) every shard's arguments are checked on the calling thread, (1) every shard reduces locally to its
// payload slot — all statuses are collected, (2) only if ALL are EC_OK does every launch thread enqueue the
// ncclAllReduce of its own communicator (the one-thread-per-device use of RCCL needs no group call), (3) copy back and
// wait.  If an enqueue of phase 2 fails on some shard after others have enqueued, the group is poisoned: its
// communicators are aborted (ncclCommAbort) so that no stream waits for the missing rank, and every later call returns
// EC_ERR_RCCL.  Every wave of every kernel launched here finishes on its own (no persistent kernels), so destroying a
// group only has to wait for its streams.
//
// The pieces: Worker and Latch (ec_worker.hpp: plain C++, so host/test_worker_queue.cpp runs the queue handshake under a thread
// sanitizer); DeviceScope (ec_runtime.hpp) puts the caller's device back; check_col / copy_col / take check and copy the per-shard
// pointer columns (the table of what is checked is at them); StreamCols holds the columns of the one-pass calls and gathers a
// shard's operands; check_program parses an expression program on the calling thread; reduce_phased is the one phased reduction.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ec_collective.hpp"
#include "ec_hostpipe.hpp"
#include "ec_lattice.hpp"
#include "ec_reclass_checks.hpp"
#include "ec_runtime.hpp"
#include "ec_worker.hpp"
#include "ec_zonal_host.hpp"

using namespace ecd;

constexpr size_t kPayloadWords = sizeof(ec_moments) / sizeof(int64_t);  // the largest payload: one stats record

struct ec_shard_group {
    int n = 0;
    uint32_t flags = 0;
    std::vector<int> devices;
    std::vector<hipStream_t> streams;
    std::vector<int64_t*> payload_dev;   // kPayloadWords per shard
    std::vector<int64_t*> payload_host;  // kPayloadWords per shard, pinned
    std::vector<ncclComm_t> comms;       // empty with EC_GROUP_HOST_COMBINE
    std::vector<Worker*> workers;        // empty when n == 1: the caller's thread does the work
    std::mutex call_mu;                  // one sharded call is POSTED at a time per group (keeps every device's queue in
                                         // call order); the synchronous calls hold it to their end (payload slots are per group)
    std::mutex err_mu;                   // first failure of a fire-and-forget job, until a sync / reduction returns it
    ec_status deferred = EC_OK;
    std::string deferred_text;
    std::atomic<bool> poisoned{false};   // a collective was left incomplete: communicators aborted, the group is unusable
    std::atomic<int64_t> posted{0};      // fire-and-forget jobs posted / run (statistics for tools/group_bench.c)
};

namespace {

using ShardFn = std::function<ec_status(int)>;

void record_deferred(ec_shard_group* g, int i, ec_status st, const std::string& text) {
    std::lock_guard<std::mutex> lk(g->err_mu);
    if (g->deferred != EC_OK) return;  // first failure wins
    g->deferred = st;
    g->deferred_text = "shard " + std::to_string(i) + " (device " + std::to_string(g->devices[i]) + "): " + text;
}

ec_status take_deferred(ec_shard_group* g) {
    std::lock_guard<std::mutex> lk(g->err_mu);
    if (g->deferred == EC_OK) return EC_OK;
    const ec_status st = g->deferred;
    g->deferred = EC_OK;
    return set_error_text(st, g->deferred_text + " (reported by a later call: the failing call had already returned)");
}

// fn(0) on the caller's thread with the group's device bound (groups of one shard have no launch threads)
ec_status run_inline(ec_shard_group* g, const ShardFn& fn) {
    DeviceScope scope;
    const ec_status st = ec_set_device(g->devices[0]);
    return st == EC_OK ? fn(0) : st;
}

// fn(i) on every shard's launch thread, concurrently; waits for all; every status is collected, the first failing one
// (and its message) is returned.
ec_status for_each_shard(ec_shard_group* g, const ShardFn& fn, std::vector<ec_status>* all = nullptr) {
    if (g->workers.empty()) {  // n == 1
        const ec_status st = run_inline(g, fn);
        if (all) all->assign(1, st);
        return st;
    }
    std::vector<ec_status> status(g->n, EC_OK);
    std::vector<std::string> text(g->n);
    Latch done(g->n);
    for (int i = 0; i < g->n; ++i) {
        g->workers[i]->post([&, i] {
            status[i] = fn(i);
            if (status[i] != EC_OK) text[i] = last_error_text();  // error text is thread-local: carry it across
            done.arrive();
        });
    }
    done.wait();
    if (all) *all = status;
    for (int i = 0; i < g->n; ++i)
        if (status[i] != EC_OK) return set_error_text(status[i], "shard " + std::to_string(i) + " (device " + std::to_string(g->devices[i]) + "): " + text[i]);
    return EC_OK;
}

// Fire-and-forget: fn owns copies of everything it needs.  Returns once the jobs are posted; failures are deferred.
ec_status post_each_shard(ec_shard_group* g, ShardFn fn) {
    if (g->flags & EC_GROUP_BLOCKING_ISSUE) return for_each_shard(g, fn);
    if (g->workers.empty()) return run_inline(g, fn);  // one shard: issuing IS the call, nothing to hand over
    auto shared = std::make_shared<ShardFn>(std::move(fn));
    for (int i = 0; i < g->n; ++i) {
        g->workers[i]->post([g, i, shared] {
            int want = i + 1;  // test hook (ec_tune_set("inject_shard_failure", shard + 1)): this job fails instead of launching
            const bool injected = tuning().inject_shard_failure.compare_exchange_strong(want, 0);
            const ec_status st = injected ? set_error(EC_ERR_HIP, "injected failure (inject_shard_failure)") : (*shared)(i);
            if (st != EC_OK) record_deferred(g, i, st, last_error_text());
        });
    }
    g->posted.fetch_add(g->n, std::memory_order_relaxed);
    return EC_OK;
}

ec_status check_group(const ec_shard_group* g, const char* what) {
    if (!g || g->n < 1) return set_error(EC_ERR_ARG, "%s: null shard group", what);
    if (g->poisoned.load(std::memory_order_acquire))
        return set_error(EC_ERR_RCCL, "%s: the shard group is poisoned (a collective was left incomplete; destroy the group)", what);
    return EC_OK;
}

// ---- the per-shard pointer columns of a call: col[i] is shard i's pointer, n[i] its cell count
// A CHECKED column has no null pointer where there are cells: it is refused on the calling thread, before any fan-out (a shard
// that failed alone would otherwise leave the others inside a collective).  What each entry point checks, in this order; the
// element-wise calls also copy their columns (they return before the launch threads read them):
//   ec_sharded_binop              l, r, out
//   ec_sharded_masked_binop       l, r, lmask, rmask, out, out_mask
//   ec_sharded_convert            src, dst
//   ec_sharded_mask_from_nodata   p, mask
//   ec_sharded_compare            l, r, lmask and rmask where given, out_mask
//   ec_sharded_compare_scalar     l, lmask where given, out_mask
//   ec_sharded_reclass            src, masks where given, tables_dev, dst, dst_masks where given
//   ec_sharded_fused              p[k] of every operand with a column, out.  NOT masks[k] and out_mask: they are copied
//                                 unchecked, a null per-shard mask reaches ec_masked_fused as it is
//   ec_sharded_expr               p[k] and (masked) masks[k] stream by stream, out, (masked) out_mask
//   ec_sharded_min_max            p, (masked) masks                            — read in place, as are the next two
//   ec_sharded_expr_min_max       p[k] and (masked) masks[k] stream by stream  — copied, for StreamCols::gather
//   ec_sharded_counts             masks
//   ec_sharded_alloc / _free / _upload / _download: no column is checked
template <typename P>
ec_status check_col(const ec_shard_group* g, const char* what, const char* name, const P* col, const size_t* n) {
    for (int i = 0; i < g->n; ++i)
        if (n[i] > 0 && !col[i]) return set_error(EC_ERR_ARG, "%s: %s[%d] is null with n[%d] = %zu", what, name, i, i, n[i]);
    return EC_OK;
}

template <typename P>
std::vector<P> copy_col(const ec_shard_group* g, const P* col) { return std::vector<P>(col, col + g->n); }

// check and copy in one step; `*st` is sticky: after a refusal nothing more is checked or copied, so a run of takes ends in one test
template <typename P>
std::vector<P> take(const ec_shard_group* g, const char* what, const char* name, const P* col, const size_t* n, ec_status* st) {
    if (*st == EC_OK) *st = check_col(g, what, name, col, n);
    return *st == EC_OK ? copy_col(g, col) : std::vector<P>();
}

// The columns of a one-pass call over up to 4 operand slots (ec_sharded_fused, ec_sharded_expr, ec_sharded_expr_min_max): an
// empty vector is a slot without a column (a scalar operand of a fused chain, a stream past the program's, an unmasked call).
struct StreamCols {
    std::vector<const void*> p[4];
    std::vector<const uint8_t*> m[4];
    std::vector<size_t> n;
    std::vector<double*> out;
    std::vector<uint8_t*> om;  // empty: no out_mask

    // shard i's operand and mask pointers, null where the slot has no column
    void gather(int i, const void* pi[4], const uint8_t* mi[4]) const {
        for (int k = 0; k < 4; ++k) {
            pi[k] = p[k].empty() ? nullptr : p[k][i];
            mi[k] = m[k].empty() ? nullptr : m[k][i];
        }
    }
};

// the program: parsed once, on the calling thread (no device needed), so that a malformed one is refused before anything is posted
ec_status check_program(const ec_dtype* dt, int32_t n_streams, int32_t n_scalars, const ec_expr_step* steps, int32_t n_steps) {
    size_t len = 0;
    return ec_expr_source(dt, n_streams, n_scalars, steps, n_steps, nullptr, nullptr, 0, &len);
}

void poison(ec_shard_group* g) {
    g->poisoned.store(true, std::memory_order_release);
    const Rccl* R = rccl("ec_shard_group(poison)");
    for (ncclComm_t c : g->comms)
        if (c && R && R->comm_abort) (void)R->comm_abort(c);  // unblocks the ranks that did enqueue
    g->comms.assign(g->comms.size(), nullptr);
}

// The exchange step of a reduction whose per-shard payloads {a, b} are in payload_dev[i][0..1] on EVERY shard
// (phase 1 succeeded everywhere).  Phase 2: every launch thread enqueues its all-reduce; phase 3: copy back, wait.
ec_status exchange(ec_shard_group* g, bool is_keys) {
    if (!g->comms.empty()) {
        std::vector<ec_status> all;
        ec_status st = for_each_shard(g, [&](int i) {
            return is_keys ? ec_allreduce_min_max_keys(g->comms[i], g->payload_dev[i], g->streams[i])
                           : ec_allreduce_counts(g->comms[i], reinterpret_cast<uint64_t*>(g->payload_dev[i]), g->streams[i]);
        }, &all);
        if (st != EC_OK) {
            bool some_enqueued = false;
            for (ec_status s : all) some_enqueued = some_enqueued || s == EC_OK;
            if (some_enqueued && g->n > 1) {
                const std::string keep = last_error_text();
                poison(g);
                return set_error_text(st, keep + " — other shards had enqueued the collective: group poisoned, communicators aborted");
            }
            return st;
        }
    }
    return for_each_shard(g, [&](int i) {
        ec_status st = check_hip(hipMemcpyAsync(g->payload_host[i], g->payload_dev[i], 2 * sizeof(int64_t), hipMemcpyDeviceToHost, g->streams[i]),
                                 "hipMemcpyAsync(payload)");
        if (st != EC_OK) return st;
        return check_hip(hipStreamSynchronize(g->streams[i]), "hipStreamSynchronize");
    });
}

enum class Combine { keys, counts };  // element-wise MAX of {~key(min), key(max)}; SUM of {n_true, n_false}

// A reduction over the group, call_mu held by the caller.  Phase 1: `local(i)` reduces shard i to payload_dev[i][0..1] (an empty
// shard contributes the idempotent payload: the sentinels (T::MAX, T::MIN) of src/buffer.rs:170, zero counts).  A failure that an
// earlier fire-and-forget call left behind comes first (its output may feed this reduction), then a failure of phase 1 — nothing
// has been enqueued on any communicator.  Only then the exchange; without communicators the host words are folded here.
ec_status reduce_phased(ec_shard_group* g, const ShardFn& local, Combine kind, int64_t out[2]) {
    ec_status st = for_each_shard(g, local);
    const std::string keep = last_error_text();
    const ec_status deferred = take_deferred(g);
    if (deferred != EC_OK) return deferred;
    if (st != EC_OK) return set_error_text(st, keep);
    if ((st = exchange(g, kind == Combine::keys)) != EC_OK) return st;
    for (int w = 0; w < 2; ++w) {
        out[w] = g->payload_host[0][w];
        for (int i = 1; g->comms.empty() && i < g->n; ++i) {
            const int64_t v = g->payload_host[i][w];
            if (kind == Combine::counts) out[w] = static_cast<int64_t>(static_cast<uint64_t>(out[w]) + static_cast<uint64_t>(v));
            else if (v > out[w]) out[w] = v;
        }
    }
    return EC_OK;
}

}  // namespace

extern "C" ec_status ec_shard_group_create(const int32_t* devices, int32_t n, uint32_t flags, ec_shard_group** out) {
    if (!devices || !out || n < 1 || n > 64) return set_error(EC_ERR_ARG, "ec_shard_group_create: null argument or n outside 1..64");
    *out = nullptr;
    const bool host_combine = (flags & EC_GROUP_HOST_COMBINE) != 0;
    if (!host_combine)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j)
                if (devices[i] == devices[j])
                    return set_error(EC_ERR_ARG, "ec_shard_group_create: device %d listed twice (RCCL needs one rank per GPU; "
                                                 "EC_GROUP_HOST_COMBINE allows it)", int(devices[i]));
    DeviceScope scope;
    std::unique_ptr<ec_shard_group> g(new ec_shard_group);
    g->n = n;
    g->flags = flags;
    g->devices.assign(devices, devices + n);
    g->streams.assign(n, nullptr);
    g->payload_dev.assign(n, nullptr);
    g->payload_host.assign(n, nullptr);
    ec_status st = EC_OK;
    for (int i = 0; i < n && st == EC_OK; ++i) {
        st = ec_init(devices[i]);
        ec_stream s = nullptr;
        if (st == EC_OK) st = ec_stream_create(&s);  // also prepares the stream's reduction scratch
        g->streams[i] = static_cast<hipStream_t>(s);
        if (st == EC_OK) st = check_hip(hipMalloc(reinterpret_cast<void**>(&g->payload_dev[i]), kPayloadWords * sizeof(int64_t)), "hipMalloc(payload)");
        if (st == EC_OK) st = check_hip(hipHostMalloc(reinterpret_cast<void**>(&g->payload_host[i]), kPayloadWords * sizeof(int64_t), hipHostMallocDefault),
                                        "hipHostMalloc(payload)");
    }
    if (st == EC_OK && !host_combine) {
        std::vector<ec_comm> cs(n, nullptr);
        st = ec_comm_init_all(devices, n, cs.data());
        if (st == EC_OK) {
            g->comms.resize(n);
            for (int i = 0; i < n; ++i) g->comms[i] = static_cast<ncclComm_t>(cs[i]);
        }
    }
    if (st == EC_OK && n > 1) {
        for (int i = 0; i < n; ++i) {
            Worker* w = new Worker;
            g->workers.push_back(w);
            w->th = std::thread([w, device = devices[i]] {
                (void)ec_set_device(device);  // for the life of the thread
                w->run();
            });
        }
    }
    if (st != EC_OK) {
        const std::string keep = last_error_text();  // why the creation failed, whatever the clean-up has to say
        (void)ec_shard_group_destroy(g.release());
        return set_error_text(st, keep);
    }
    *out = g.release();
    return EC_OK;
}

extern "C" ec_status ec_shard_group_destroy(ec_shard_group* g) {
    if (!g) return EC_OK;
    for (Worker* w : g->workers) {
        w->stop_and_join();  // runs what is still queued
        delete w;
    }
    g->workers.clear();
    DeviceScope scope;
    for (int i = 0; i < g->n; ++i) {
        if (ec_set_device(g->devices[i]) != EC_OK) continue;
        if (g->streams[i]) (void)hipStreamSynchronize(g->streams[i]);
        if (i < int(g->comms.size()) && g->comms[i]) (void)ec_comm_destroy(g->comms[i]);
        if (g->payload_dev[i]) (void)hipFree(g->payload_dev[i]);
        if (g->payload_host[i]) (void)hipHostFree(g->payload_host[i]);
        if (g->streams[i]) (void)ec_stream_destroy(g->streams[i]);
    }
    delete g;
    return EC_OK;
}

extern "C" int32_t ec_shard_group_size(const ec_shard_group* g) { return g ? g->n : 0; }

extern "C" ec_status ec_shard_group_shard(const ec_shard_group* g, int32_t shard, int32_t* device, ec_stream* stream) {
    ec_status st = check_group(g, "ec_shard_group_shard");
    if (st != EC_OK) return st;
    if (shard < 0 || shard >= g->n) return set_error(EC_ERR_ARG, "ec_shard_group_shard: shard %d of %d", int(shard), g->n);
    if (device) *device = g->devices[shard];
    if (stream) *stream = g->streams[shard];
    return EC_OK;
}

extern "C" ec_status ec_shard_group_foreach(ec_shard_group* g, ec_shard_fn fn, void* user) {
    ec_status st = check_group(g, "ec_shard_group_foreach");
    if (st != EC_OK) return st;
    if (!fn) return set_error(EC_ERR_ARG, "ec_shard_group_foreach: null callback");
    std::lock_guard<std::mutex> lk(g->call_mu);
    return for_each_shard(g, [&](int i) { return fn(i, g->devices[i], g->streams[i], user); });
}

// Waits until every posted job has been issued and every shard's stream has drained; returns the first failure a
// fire-and-forget call left behind (and clears it), else the streams' own status.
extern "C" ec_status ec_shard_group_sync(ec_shard_group* g) {
    if (!g || g->n < 1) return set_error(EC_ERR_ARG, "ec_shard_group_sync: null shard group");
    std::lock_guard<std::mutex> lk(g->call_mu);
    const ec_status st = for_each_shard(g, [&](int i) { return check_hip(hipStreamSynchronize(g->streams[i]), "hipStreamSynchronize"); });
    const std::string keep = last_error_text();
    const ec_status deferred = take_deferred(g);
    if (deferred != EC_OK) return deferred;
    if (st != EC_OK) return set_error_text(st, keep);
    return check_group(g, "ec_shard_group_sync");  // a poisoned group says so
}

extern "C" ec_status ec_shard_group_stat(const ec_shard_group* g, const char* key, int64_t* value) {
    if (!g || !key || !value) return set_error(EC_ERR_ARG, "ec_shard_group_stat: null argument");
    if (!std::strcmp(key, "jobs_posted")) *value = g->posted.load(std::memory_order_relaxed);
    else if (!std::strcmp(key, "poisoned")) *value = g->poisoned.load(std::memory_order_acquire) ? 1 : 0;
    else if (!std::strcmp(key, "blocking_issue")) *value = (g->flags & EC_GROUP_BLOCKING_ISSUE) ? 1 : 0;
    else return set_error(EC_ERR_ARG, "ec_shard_group_stat: unknown key '%s'", key);
    return EC_OK;
}

extern "C" ec_status ec_sharded_alloc(ec_shard_group* g, const size_t* bytes, void** dptrs) {
    ec_status st = check_group(g, "ec_sharded_alloc");
    if (st != EC_OK) return st;
    if (!bytes || !dptrs) return set_error(EC_ERR_ARG, "ec_sharded_alloc: null argument");
    for (int i = 0; i < g->n; ++i) dptrs[i] = nullptr;
    std::lock_guard<std::mutex> lk(g->call_mu);
    st = for_each_shard(g, [&](int i) { return ec_alloc(&dptrs[i], bytes[i]); });
    if (st != EC_OK) {
        const std::string keep = last_error_text();
        (void)for_each_shard(g, [&](int i) { ec_status f = ec_free(dptrs[i]); dptrs[i] = nullptr; return f; });
        return set_error_text(st, keep);
    }
    return EC_OK;
}

// (queued behind the launches posted so far on each device; hipFree then waits for the device)
extern "C" ec_status ec_sharded_free(ec_shard_group* g, void* const* dptrs) {
    if (!g || g->n < 1) return set_error(EC_ERR_ARG, "ec_sharded_free: null shard group");  // a poisoned group still frees
    if (!dptrs) return set_error(EC_ERR_ARG, "ec_sharded_free: null argument");
    std::lock_guard<std::mutex> lk(g->call_mu);
    return for_each_shard(g, [&](int i) { return ec_free(dptrs[i]); });
}

extern "C" ec_status ec_sharded_upload(ec_shard_group* g, void* const* dst_dev, const void* src_host,
                                       const size_t* byte_offsets, const size_t* bytes) {
    ec_status st = check_group(g, "ec_sharded_upload");
    if (st != EC_OK) return st;
    if (!dst_dev || !byte_offsets || !bytes) return set_error(EC_ERR_ARG, "ec_sharded_upload: null argument");
    std::lock_guard<std::mutex> lk(g->call_mu);
    return for_each_shard(g, [&](int i) {
        return ec_upload(dst_dev[i], static_cast<const char*>(src_host) + byte_offsets[i], bytes[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_download(ec_shard_group* g, void* dst_host, const void* const* src_dev,
                                         const size_t* byte_offsets, const size_t* bytes) {
    ec_status st = check_group(g, "ec_sharded_download");
    if (st != EC_OK) return st;
    if (!src_dev || !byte_offsets || !bytes) return set_error(EC_ERR_ARG, "ec_sharded_download: null argument");
    std::lock_guard<std::mutex> lk(g->call_mu);
    return for_each_shard(g, [&](int i) {
        return ec_download(static_cast<char*>(dst_host) + byte_offsets[i], src_dev[i], bytes[i], g->streams[i]);
    });
}

// ---- element-wise: checked on the calling thread, posted, not waited for
extern "C" ec_status ec_sharded_binop(ec_shard_group* g, ec_op op, ec_dtype lt, const void* const* l, ec_dtype rt,
                                      const void* const* r, const size_t* n, double* const* out) {
    ec_status st = check_group(g, "ec_sharded_binop");
    if (st != EC_OK) return st;
    if (!l || !r || !n || !out) return set_error(EC_ERR_ARG, "ec_sharded_binop: null argument");
    if (op < EC_ADD || op > EC_DIV) return set_error(EC_ERR_ARG, "ec_sharded_binop: bad op");
    if (!ecl::valid(lt) || !ecl::valid(rt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_sharded_binop: bad dtype");
    const char* what = "ec_sharded_binop";
    auto lv = take(g, what, "l", l, n, &st);
    auto rv = take(g, what, "r", r, n, &st);
    auto ov = take(g, what, "out", out, n, &st);
    if (st != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, op, lt, rt, l = std::move(lv), r = std::move(rv), n = copy_col(g, n), out = std::move(ov)](int i) {
        return ec_binop(op, lt, l[i], rt, r[i], n[i], out[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_masked_binop(ec_shard_group* g, ec_op op, ec_dtype lt, const void* const* l, const uint8_t* const* lmask,
                                             ec_dtype rt, const void* const* r, const uint8_t* const* rmask, const size_t* n,
                                             double* const* out, uint8_t* const* out_mask) {
    ec_status st = check_group(g, "ec_sharded_masked_binop");
    if (st != EC_OK) return st;
    if (!l || !lmask || !r || !rmask || !n || !out || !out_mask) return set_error(EC_ERR_ARG, "ec_sharded_masked_binop: null argument");
    if (op < EC_ADD || op > EC_DIV) return set_error(EC_ERR_ARG, "ec_sharded_masked_binop: bad op");
    if (!ecl::valid(lt) || !ecl::valid(rt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_sharded_masked_binop: bad dtype");
    const char* what = "ec_sharded_masked_binop";
    auto lv = take(g, what, "l", l, n, &st);
    auto rv = take(g, what, "r", r, n, &st);
    auto lmv = take(g, what, "lmask", lmask, n, &st);
    auto rmv = take(g, what, "rmask", rmask, n, &st);
    auto ov = take(g, what, "out", out, n, &st);
    auto omv = take(g, what, "out_mask", out_mask, n, &st);
    if (st != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, op, lt, rt, l = std::move(lv), lm = std::move(lmv), r = std::move(rv), rm = std::move(rmv),
                               n = copy_col(g, n), out = std::move(ov), om = std::move(omv)](int i) {
        return ec_masked_binop(op, lt, l[i], lm[i], rt, r[i], rm[i], n[i], out[i], om[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_convert(ec_shard_group* g, ec_dtype st_, const void* const* src, ec_dtype dt, void* const* dst,
                                        const size_t* n) {
    ec_status st = check_group(g, "ec_sharded_convert");
    if (st != EC_OK) return st;
    if (!ecl::valid(st_) || !ecl::valid(dt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_sharded_convert: bad dtype");
    if (!ec_can_fit_into(st_, dt)) return ec_convert(st_, nullptr, dt, nullptr, 0, nullptr);  // EC_ERR_NARROWING, before any device work
    if (!src || !dst || !n) return set_error(EC_ERR_ARG, "ec_sharded_convert: null argument");
    auto sv = take(g, "ec_sharded_convert", "src", src, n, &st);
    auto dv = take(g, "ec_sharded_convert", "dst", dst, n, &st);
    if (st != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, st_, dt, src = std::move(sv), dst = std::move(dv), n = copy_col(g, n)](int i) {
        return ec_convert(st_, src[i], dt, dst[i], n[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_mask_from_nodata(ec_shard_group* g, ec_dtype t, const void* const* p, const size_t* n,
                                                 const ec_value* nd_or_null, uint8_t* const* mask) {
    ec_status st = check_group(g, "ec_sharded_mask_from_nodata");
    if (st != EC_OK) return st;
    if (!p || !n || !mask) return set_error(EC_ERR_ARG, "ec_sharded_mask_from_nodata: null argument");
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_sharded_mask_from_nodata: bad dtype");
    auto pv = take(g, "ec_sharded_mask_from_nodata", "p", p, n, &st);
    auto mv = take(g, "ec_sharded_mask_from_nodata", "mask", mask, n, &st);
    if (st != EC_OK) return st;
    const bool has_nd = nd_or_null != nullptr;
    const ec_value nd = has_nd ? *nd_or_null : ec_value{};
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, t, has_nd, nd, p = std::move(pv), n = copy_col(g, n), mask = std::move(mv)](int i) {
        return ec_mask_from_nodata(t, p[i], n[i], has_nd ? &nd : nullptr, mask[i], g->streams[i]);
    });
}

// an optional mask column: checked and copied when given, a column of nulls otherwise
static std::vector<const uint8_t*> take_optional(const ec_shard_group* g, const char* what, const char* name, const uint8_t* const* col,
                                                 const size_t* n, ec_status* st) {
    return col ? take(g, what, name, col, n, st) : std::vector<const uint8_t*>(g->n, nullptr);
}

extern "C" ec_status ec_sharded_compare(ec_shard_group* g, int32_t rel, ec_dtype lt, const void* const* l, const uint8_t* const* lmask_or_null,
                                        ec_dtype rt, const void* const* r, const uint8_t* const* rmask_or_null, const size_t* n,
                                        uint8_t* const* out_mask) {
    const char* what = "ec_sharded_compare";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    st = ec_compare(rel, lt, nullptr, nullptr, rt, nullptr, nullptr, 0, nullptr, nullptr);  // relation and dtypes, before any device work
    if (st != EC_OK) return st;
    if (!l || !r || !n || !out_mask) return set_error(EC_ERR_ARG, "%s: null argument", what);
    auto lv = take(g, what, "l", l, n, &st);
    auto rv = take(g, what, "r", r, n, &st);
    auto lmv = take_optional(g, what, "lmask", lmask_or_null, n, &st);
    auto rmv = take_optional(g, what, "rmask", rmask_or_null, n, &st);
    auto ov = take(g, what, "out_mask", out_mask, n, &st);
    if (st != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, rel, lt, rt, l = std::move(lv), lm = std::move(lmv), r = std::move(rv), rm = std::move(rmv),
                               n = copy_col(g, n), out = std::move(ov)](int i) {
        return ec_compare(rel, lt, l[i], lm[i], rt, r[i], rm[i], n[i], out[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_compare_scalar(ec_shard_group* g, int32_t rel, ec_dtype lt, const void* const* l,
                                               const uint8_t* const* lmask_or_null, const size_t* n, const ec_value* rhs,
                                               uint8_t* const* out_mask) {
    const char* what = "ec_sharded_compare_scalar";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    st = ec_compare_scalar(rel, lt, nullptr, nullptr, 0, rhs, nullptr, nullptr);  // relation, scalar and dtypes, before any device work
    if (st != EC_OK) return st;
    if (!l || !n || !out_mask) return set_error(EC_ERR_ARG, "%s: null argument", what);
    auto lv = take(g, what, "l", l, n, &st);
    auto lmv = take_optional(g, what, "lmask", lmask_or_null, n, &st);
    auto ov = take(g, what, "out_mask", out_mask, n, &st);
    if (st != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, rel, lt, rhs = *rhs, l = std::move(lv), lm = std::move(lmv), n = copy_col(g, n), out = std::move(ov)](int i) {
        return ec_compare_scalar(rel, lt, l[i], lm[i], n[i], &rhs, out[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_cast(ec_shard_group* g, int32_t mode, ec_dtype st_, const void* const* src, ec_dtype dt, void* const* dst,
                                     const size_t* n) {
    const char* what = "ec_sharded_cast";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    st = ec_cast(mode, st_, nullptr, dt, nullptr, 0, nullptr);  // mode and dtypes, before any device work
    if (st != EC_OK) return st;
    if (!src || !dst || !n) return set_error(EC_ERR_ARG, "%s: null argument", what);
    auto sv = take(g, what, "src", src, n, &st);
    auto dv = take(g, what, "dst", dst, n, &st);
    if (st != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, mode, st_, dt, src = std::move(sv), dst = std::move(dv), n = copy_col(g, n)](int i) {
        return ec_cast(mode, st_, src[i], dt, dst[i], n[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_cast_scaled(ec_shard_group* g, ec_dtype st_, const void* const* src, const uint8_t* const* masks_or_null,
                                            const size_t* n, double scale, double offset, ec_dtype dt, const ec_value* nodata_or_null,
                                            void* const* dst) {
    const char* what = "ec_sharded_cast_scaled";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    // the pairing of masks and nodata, its dtype, the dtypes, scale and offset, before any device work (n = 0: nothing is read)
    st = ec_cast_scaled(st_, nullptr, reinterpret_cast<const uint8_t*>(masks_or_null), 0, scale, offset, dt, nodata_or_null, nullptr, nullptr);
    if (st != EC_OK) return st;
    if (!src || !dst || !n) return set_error(EC_ERR_ARG, "%s: null argument", what);
    auto sv = take(g, what, "src", src, n, &st);
    auto mv = take_optional(g, what, "masks", masks_or_null, n, &st);
    auto dv = take(g, what, "dst", dst, n, &st);
    if (st != EC_OK) return st;
    const bool masked = nodata_or_null != nullptr;
    const ec_value nd = masked ? *nodata_or_null : ec_value{};
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, st_, dt, scale, offset, masked, nd, src = std::move(sv), m = std::move(mv), dst = std::move(dv),
                               n = copy_col(g, n)](int i) -> ec_status {
        if (n[i] == 0) return EC_OK;  // an empty shard may have no mask pointer: not the "mask without nodata" refusal
        return ec_cast_scaled(st_, src[i], m[i], n[i], scale, offset, dt, masked ? &nd : nullptr, dst[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_reclass(ec_shard_group* g, ec_dtype t, const void* const* src, const uint8_t* const* masks_or_null, const size_t* n,
                                        ec_dtype dt, const void* const* tables_dev, void* const* dst, uint8_t* const* dst_masks_or_null) {
    const char* what = "ec_sharded_reclass";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    st = ec_reclass(t, nullptr, nullptr, 0, dt, nullptr, nullptr, nullptr, nullptr);  // the dtypes, before any device work
    if (st != EC_OK) return st;
    if (!src || !tables_dev || !dst || !n) return set_error(EC_ERR_ARG, "%s: null argument", what);
    auto sv = take(g, what, "src", src, n, &st);
    auto mv = take_optional(g, what, "masks", masks_or_null, n, &st);
    auto tv = take(g, what, "tables_dev", tables_dev, n, &st);
    auto dv = take(g, what, "dst", dst, n, &st);
    auto omv = dst_masks_or_null ? take(g, what, "dst_masks", dst_masks_or_null, n, &st) : std::vector<uint8_t*>(g->n, nullptr);
    if (st != EC_OK) return st;
    for (int i = 0; i < g->n; ++i) {  // every shard's own refusals of ec_reclass, here: nothing is posted after one
        if (const ecv::Refusal r = ecr::reclass_refusal(ecl::size_of(t), ecl::size_of(dt), sv[i], mv[i], n[i], tv[i], dv[i], omv[i]))
            return set_error(EC_ERR_ARG, "%s: shard %d: %s", what, i, r.why);
    }
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, t, dt, src = std::move(sv), m = std::move(mv), tab = std::move(tv), dst = std::move(dv), om = std::move(omv),
                               n = copy_col(g, n)](int i) {
        return ec_reclass(t, src[i], m[i], n[i], dt, tab[i], dst[i], om[i], g->streams[i]);
    });
}

// A stack call (ec_sharded_composite, ec_sharded_composite_rank) behind its group check and its pre-check: the columns are checked
// and copied on the calling thread, then shard i's job gathers its K layer and mask pointers and hands them to `each`, which makes
// the unsharded call: each(p, m, n, dst, dst_mask, aux, stream).  A refused call posts nothing.
template <typename Each>
static ec_status post_stack(ec_shard_group* g, const char* what, const void* const* const* layers, const uint8_t* const* const* masks_or_null,
                            int32_t n_layers, const size_t* n, void* const* dst, uint8_t* const* dst_mask_or_null, uint8_t* const* aux_or_null,
                            Each each) {
    if (!layers || !dst || !n) return set_error(EC_ERR_ARG, "%s: null argument", what);
    struct Call {
        std::vector<const void*> p[64];
        std::vector<const uint8_t*> m[64];
        std::vector<void*> dst;
        std::vector<uint8_t*> dm, aux;
        std::vector<size_t> n;
    };
    auto c = std::make_shared<Call>();
    bool masked = false;
    for (int k = 0; k < n_layers; ++k) {
        if (!layers[k]) return set_error(EC_ERR_ARG, "%s: layer %d is a null column", what, k);
        masked = masked || (masks_or_null && masks_or_null[k]);
    }
    if (masked && !dst_mask_or_null) return set_error(EC_ERR_ARG, "%s: a layer has a mask, so the result needs dst_mask", what);
    ec_status st = EC_OK;
    for (int k = 0; k < n_layers; ++k) {
        c->p[k] = take(g, what, "layers[k]", layers[k], n, &st);
        c->m[k] = take_optional(g, what, "masks[k]", masks_or_null ? masks_or_null[k] : nullptr, n, &st);
    }
    c->dst = take(g, what, "dst", dst, n, &st);
    if (dst_mask_or_null) c->dm = take(g, what, "dst_mask", dst_mask_or_null, n, &st);
    if (aux_or_null) c->aux = take(g, what, "aux", aux_or_null, n, &st);
    if (st != EC_OK) return st;
    c->n = copy_col(g, n);
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, c, n_layers, each](int i) -> ec_status {
        const void* p[64];
        const uint8_t* m[64];
        for (int k = 0; k < n_layers; ++k) {
            p[k] = c->p[k][i];
            m[k] = c->m[k][i];
        }
        return each(p, m, c->n[i], c->dst[i], c->dm.empty() ? nullptr : c->dm[i], c->aux.empty() ? nullptr : c->aux[i], g->streams[i]);
    });
}

extern "C" ec_status ec_sharded_composite(ec_shard_group* g, int32_t op, ec_dtype t, const void* const* const* layers,
                                          const uint8_t* const* const* masks_or_null, int32_t n_layers, const size_t* n, uint32_t min_count,
                                          void* const* dst, uint8_t* const* dst_mask_or_null, uint8_t* const* aux_or_null) {
    const char* what = "ec_sharded_composite";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    // the op, the layer count, min_count and the dtype, before any device work (n = 0: no pointer is looked at)
    st = ec_composite(op, t, nullptr, nullptr, n_layers, 0, min_count, nullptr, nullptr, nullptr, nullptr);
    if (st != EC_OK) return st;
    return post_stack(g, what, layers, masks_or_null, n_layers, n, dst, dst_mask_or_null, aux_or_null,
                      [=](const void* const* p, const uint8_t* const* m, size_t ni, void* d, uint8_t* dm, uint8_t* aux, ec_stream s) {
                          return ec_composite(op, t, p, m, n_layers, ni, min_count, d, dm, aux, s);
                      });
}

extern "C" ec_status ec_sharded_composite_rank(ec_shard_group* g, ec_dtype t, const void* const* const* layers,
                                               const uint8_t* const* const* masks_or_null, int32_t n_layers, const size_t* n, uint32_t num,
                                               uint32_t den, int32_t method, uint32_t min_count, void* const* dst,
                                               uint8_t* const* dst_mask_or_null, uint8_t* const* aux_or_null) {
    const char* what = "ec_sharded_composite_rank";
    ec_status st = check_group(g, what);
    if (st != EC_OK) return st;
    // the layer count, q, the method, min_count and the dtype, before any device work (n = 0: no pointer is looked at)
    st = ec_composite_rank(t, nullptr, nullptr, n_layers, 0, num, den, method, min_count, nullptr, nullptr, nullptr, nullptr);
    if (st != EC_OK) return st;
    return post_stack(g, what, layers, masks_or_null, n_layers, n, dst, dst_mask_or_null, aux_or_null,
                      [=](const void* const* p, const uint8_t* const* m, size_t ni, void* d, uint8_t* dm, uint8_t* aux, ec_stream s) {
                          return ec_composite_rank(t, p, m, n_layers, ni, num, den, method, min_count, d, dm, aux, s);
                      });
}

extern "C" ec_status ec_sharded_fused(ec_shard_group* g, ec_op o1, ec_op o2, ec_op o3, const ec_dtype dt[4], const void* const* const p[4],
                                      const uint8_t* const* const masks_or_null[4], const ec_value* scalars_or_null, const size_t* n,
                                      double* const* out, uint8_t* const* out_mask_or_null) {
    ec_status st = check_group(g, "ec_sharded_fused");
    if (st != EC_OK) return st;
    if (!dt || !p || !n || !out) return set_error(EC_ERR_ARG, "ec_sharded_fused: null argument");
    if ((masks_or_null != nullptr) != (out_mask_or_null != nullptr))
        return set_error(EC_ERR_ARG, "ec_sharded_fused: masks and out_mask go together");
    const int nops = o3 == static_cast<ec_op>(-1) ? 3 : 4;
    struct Call : StreamCols {
        ec_op o1, o2, o3;
        ec_dtype dt[4];
        bool masked, has_sc;
        ec_value sc[4];
    };
    auto c = std::make_shared<Call>();
    c->o1 = o1; c->o2 = o2; c->o3 = o3;
    c->masked = masks_or_null != nullptr;
    c->has_sc = scalars_or_null != nullptr;
    for (int k = 0; k < 4; ++k) {
        c->dt[k] = dt[k];
        c->sc[k] = scalars_or_null ? scalars_or_null[k] : ec_value{};
        if (k >= nops || !p[k]) continue;  // no pointer array: operand k is the scalar scalars[k]
        c->p[k] = take(g, "ec_sharded_fused", "p[k]", p[k], n, &st);
        if (st != EC_OK) return st;
        if (masks_or_null && masks_or_null[k]) c->m[k] = copy_col(g, masks_or_null[k]);  // unchecked (see the table)
    }
    c->out = take(g, "ec_sharded_fused", "out", out, n, &st);
    if (st != EC_OK) return st;
    c->n = copy_col(g, n);
    if (out_mask_or_null) c->om = copy_col(g, out_mask_or_null);  // unchecked
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, c](int i) {
        const void* pi[4];
        const uint8_t* mi[4];
        c->gather(i, pi, mi);
        const ec_value* sc = c->has_sc ? c->sc : nullptr;
        if (c->masked) return ec_masked_fused(c->o1, c->o2, c->o3, c->dt, pi, mi, sc, c->n[i], c->out[i], c->om[i], g->streams[i]);
        return ec_fused(c->o1, c->o2, c->o3, c->dt, pi, sc, c->n[i], c->out[i], g->streams[i]);
    });
}

// Expression programs (ec_expr / ec_masked_expr) on every shard.  p[k] / masks_or_null[k]: stream k's per-shard pointers.
// Everything that can be refused is refused here, on the calling thread, the program included.
extern "C" ec_status ec_sharded_expr(ec_shard_group* g, const ec_dtype* dt, const void* const* const* p,
                                     const uint8_t* const* const* masks_or_null, int32_t n_streams, const ec_value* scalars,
                                     int32_t n_scalars, const ec_expr_step* steps, int32_t n_steps, const size_t* n, double* const* out,
                                     uint8_t* const* out_mask_or_null) {
    ec_status st = check_group(g, "ec_sharded_expr");
    if (st != EC_OK) return st;
    if (!dt || !p || !steps || !n || !out || (n_scalars > 0 && !scalars)) return set_error(EC_ERR_ARG, "ec_sharded_expr: null argument");
    if (n_streams < 1 || n_streams > 4 || n_scalars < 0 || n_scalars > 8 || n_steps < 1 || n_steps > 16)
        return set_error(EC_ERR_ARG, "ec_sharded_expr: %d streams (1..4), %d scalars (0..8), %d steps (1..16)", int(n_streams), int(n_scalars), int(n_steps));
    if ((masks_or_null != nullptr) != (out_mask_or_null != nullptr)) return set_error(EC_ERR_ARG, "ec_sharded_expr: masks and out_mask go together");
    if ((st = check_program(dt, n_streams, n_scalars, steps, n_steps)) != EC_OK) return st;
    struct Call : StreamCols {
        int32_t ns, nsc, nst;
        ec_dtype dt[4];
        ec_value sc[8];
        ec_expr_step steps[16];
        bool masked;
    };
    auto c = std::make_shared<Call>();
    c->ns = n_streams; c->nsc = n_scalars; c->nst = n_steps;
    c->masked = masks_or_null != nullptr;
    for (int k = 0; k < n_streams; ++k) {
        c->dt[k] = dt[k];
        if (!p[k] || (c->masked && !masks_or_null[k])) return set_error(EC_ERR_ARG, "ec_sharded_expr: stream %d has no pointer array", k);
        c->p[k] = take(g, "ec_sharded_expr", "p[k]", p[k], n, &st);
        if (c->masked) c->m[k] = take(g, "ec_sharded_expr", "masks[k]", masks_or_null[k], n, &st);
        if (st != EC_OK) return st;  // before the next stream's own refusal
    }
    for (int k = 0; k < n_scalars; ++k) c->sc[k] = scalars[k];
    for (int k = 0; k < n_steps; ++k) c->steps[k] = steps[k];
    c->out = take(g, "ec_sharded_expr", "out", out, n, &st);
    if (out_mask_or_null) c->om = take(g, "ec_sharded_expr", "out_mask", out_mask_or_null, n, &st);
    if (st != EC_OK) return st;
    c->n = copy_col(g, n);
    std::lock_guard<std::mutex> lk(g->call_mu);
    return post_each_shard(g, [g, c](int i) {
        const void* pi[4];
        const uint8_t* mi[4];
        c->gather(i, pi, mi);
        if (c->masked) return ec_masked_expr(c->dt, pi, mi, c->ns, c->sc, c->nsc, c->steps, c->nst, c->n[i], c->out[i], c->om[i], g->streams[i]);
        return ec_expr(c->dt, pi, c->ns, c->sc, c->nsc, c->steps, c->nst, c->n[i], c->out[i], g->streams[i]);
    });
}

// Host memory in, host memory out over ALL the GPUs of the group: the raster's row-blocks (ec_shard_range) go through
// ec_host_expr / ec_host_masked_expr side by side, one pipeline per launch thread — every GPU has its own PCIe link, so a
// host-resident raster is bound by the sum of the links (and then by host memory), not by one of them.  Synchronous.
extern "C" ec_status ec_sharded_host_expr(ec_shard_group* g, const ec_dtype* dt, const void* const* p_host, const ec_value* const* nodata_or_null,
                                          int32_t n_streams, const ec_value* scalars, int32_t n_scalars, const ec_expr_step* steps, int32_t n_steps,
                                          uint64_t n_rows, uint64_t n_cols, double* out_host, const double* out_nodata_or_null,
                                          uint8_t* out_mask_host_or_null, size_t chunk_cells) {
    ec_status st = check_group(g, "ec_sharded_host_expr");
    if (st != EC_OK) return st;
    if (!dt || !p_host || !steps || !out_host) return set_error(EC_ERR_ARG, "ec_sharded_host_expr: null argument");
    if ((st = check_program(dt, n_streams, n_scalars, steps, n_steps)) != EC_OK) return st;
    for (int k = 0; k < n_streams; ++k)
        if (!p_host[k]) return set_error(EC_ERR_ARG, "ec_sharded_host_expr: stream %d is null", k);
    // everything a shard's pipeline would refuse is refused here, on the calling thread, before a page is locked
    if (nodata_or_null)
        for (int k = 0; k < n_streams; ++k)
            if (nodata_or_null[k] && nodata_or_null[k]->dtype != dt[k])
                return set_error(EC_ERR_ARG, "ec_sharded_host_expr: nodata[%d] has cell type %d, its stream %d", k, int(nodata_or_null[k]->dtype), int(dt[k]));
    if (n_cols != 0 && n_rows > (UINT64_MAX / 8) / n_cols)  // n cells of at most 8 bytes: the byte counts below stay inside 64 bits
        return set_error(EC_ERR_ARG, "ec_sharded_host_expr: %llu x %llu cells overflow the address space", (unsigned long long)n_rows, (unsigned long long)n_cols);
    if ((st = ensure_ready()) != EC_OK) return st;
    // the WHOLE arrays are page-locked once, here; the shards' pipelines find their row-blocks inside these registrations
    // (row-blocks end in the middle of pages: registering them one by one would collide on the shared pages).  Arrays the runtime
    // refuses to register stay in the table as ranges in use; the shards share those entries and copy
    // through the pageable path (PinSet, ec_hostpipe.hip)
    const uint64_t n = n_rows * n_cols;
    PinSet whole;
    {
        std::vector<std::pair<const void*, size_t>> ranges;
        for (int k = 0; k < n_streams; ++k) ranges.emplace_back(p_host[k], n * ecl::size_of(dt[k]));
        ranges.emplace_back(out_host, n * sizeof(double));
        if (out_mask_host_or_null) ranges.emplace_back(out_mask_host_or_null, n);
        // small rasters are not registered at all (ec_hostpipe.hip: their pages are shared heap pages the runtime pins itself); the shards'
        // pipelines decide the same way, each for its row-block
        size_t link = 0;
        for (const auto& r : ranges) link += r.second;
        if (link > (size_t(64) << 20)) whole.pin_all(ranges);
        else whole.use_all(ranges);
    }
    std::lock_guard<std::mutex> lk(g->call_mu);
    return for_each_shard(g, [&](int i) {
        uint64_t off = 0, len = 0;
        ec_status s = ec_shard_range(n_rows, n_cols, static_cast<uint32_t>(i), static_cast<uint32_t>(g->n), &off, &len);
        if (s != EC_OK || len == 0) return s;
        const void* p[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < n_streams; ++k) p[k] = static_cast<const char*>(p_host[k]) + off * ecl::size_of(dt[k]);
        if (nodata_or_null)
            return ec_host_masked_expr(dt, p, nodata_or_null, n_streams, scalars, n_scalars, steps, n_steps, len, out_host + off, out_nodata_or_null,
                                       out_mask_host_or_null ? out_mask_host_or_null + off : nullptr, chunk_cells);
        return ec_host_expr(dt, p, n_streams, scalars, n_scalars, steps, n_steps, len, out_host + off, chunk_cells);
    });
}

// ---- reductions: synchronous, phased (see the head of this file)
extern "C" ec_status ec_sharded_min_max(ec_shard_group* g, ec_dtype t, const void* const* p, const uint8_t* const* masks_or_null,
                                        const size_t* n, ec_value* mn, ec_value* mx) {
    ec_status st = check_group(g, "ec_sharded_min_max");
    if (st != EC_OK) return st;
    if (!p || !n || !mn || !mx) return set_error(EC_ERR_ARG, "ec_sharded_min_max: null argument");
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_sharded_min_max: bad dtype");
    if ((st = check_col(g, "ec_sharded_min_max", "p", p, n)) != EC_OK) return st;
    if (masks_or_null && (st = check_col(g, "ec_sharded_min_max", "masks", masks_or_null, n)) != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    int64_t keys[2];
    st = reduce_phased(g, [&](int i) {
        return ec_min_max_keys(t, p[i], masks_or_null ? masks_or_null[i] : nullptr, n[i], g->payload_dev[i], g->streams[i]);
    }, Combine::keys, keys);
    return st == EC_OK ? ec_min_max_decode(t, keys, mn, mx) : st;
}

// min_max of an expression program's result over the whole sharded raster, without the raster: ec_expr_min_max_keys per shard
// (the compiled reduce kernel, or two passes until the program is compiled), then the same 16-byte MAX exchange as
// ec_sharded_min_max.  Synchronous, phased like the other reductions.
extern "C" ec_status ec_sharded_expr_min_max(ec_shard_group* g, const ec_dtype* dt, const void* const* const* p,
                                             const uint8_t* const* const* masks_or_null, int32_t n_streams, const ec_value* scalars,
                                             int32_t n_scalars, const ec_expr_step* steps, int32_t n_steps, const size_t* n, ec_value* mn,
                                             ec_value* mx) {
    ec_status st = check_group(g, "ec_sharded_expr_min_max");
    if (st != EC_OK) return st;
    if (!dt || !p || !steps || !n || !mn || !mx || (n_scalars > 0 && !scalars)) return set_error(EC_ERR_ARG, "ec_sharded_expr_min_max: null argument");
    if ((st = check_program(dt, n_streams, n_scalars, steps, n_steps)) != EC_OK) return st;
    StreamCols c;  // operand and mask columns only
    for (int k = 0; k < n_streams; ++k) {
        if (!p[k] || (masks_or_null && !masks_or_null[k])) return set_error(EC_ERR_ARG, "ec_sharded_expr_min_max: stream %d has no pointer array", k);
        c.p[k] = take(g, "ec_sharded_expr_min_max", "p[k]", p[k], n, &st);
        if (masks_or_null) c.m[k] = take(g, "ec_sharded_expr_min_max", "masks[k]", masks_or_null[k], n, &st);
        if (st != EC_OK) return st;
    }
    std::lock_guard<std::mutex> lk(g->call_mu);
    int64_t keys[2];
    st = reduce_phased(g, [&](int i) {
        const void* pi[4];
        const uint8_t* mi[4];
        c.gather(i, pi, mi);
        return ec_expr_min_max_keys(dt, pi, masks_or_null ? mi : nullptr, n_streams, scalars, n_scalars, steps, n_steps, n[i], g->payload_dev[i], g->streams[i]);
    }, Combine::keys, keys);
    return st == EC_OK ? ec_min_max_decode(EC_F64, keys, mn, mx) : st;
}

extern "C" ec_status ec_sharded_counts(ec_shard_group* g, const uint8_t* const* masks, const size_t* n, uint64_t* n_true,
                                       uint64_t* n_false) {
    ec_status st = check_group(g, "ec_sharded_counts");
    if (st != EC_OK) return st;
    if (!masks || !n || !n_true || !n_false) return set_error(EC_ERR_ARG, "ec_sharded_counts: null argument");
    if ((st = check_col(g, "ec_sharded_counts", "masks", masks, n)) != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    int64_t sums[2];
    st = reduce_phased(g, [&](int i) {
        return ec_mask_counts_device(masks[i], n[i], reinterpret_cast<uint64_t*>(g->payload_dev[i]), g->streams[i]);
    }, Combine::counts, sums);
    if (st != EC_OK) return st;
    *n_true = static_cast<uint64_t>(sums[0]);
    *n_false = static_cast<uint64_t>(sums[1]);
    return EC_OK;
}

// Band statistics of the whole raster (ec_stats_device per shard; BufferOps::min_max, src/buffer.rs:169-173, with the moments
// beside it): every shard writes its 64-byte record to its payload slot, the records come down and ec_stats_fold folds them in
// shard order on the host.  No collective — nothing to poison, the same bits on every run, no RCCL.  Phased like the other
// reductions as far as it goes: arguments first, then every shard's launch, and a failure an earlier call left behind comes first.
extern "C" ec_status ec_sharded_stats(ec_shard_group* g, ec_dtype t, const void* const* p, const uint8_t* const* masks_or_null,
                                      const size_t* n, void* stats_out) {
    ec_status st = check_group(g, "ec_sharded_stats");
    if (st != EC_OK) return st;
    if (!p || !n || !stats_out) return set_error(EC_ERR_ARG, "ec_sharded_stats: null argument");
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_sharded_stats: bad dtype");
    if ((st = check_col(g, "ec_sharded_stats", "p", p, n)) != EC_OK) return st;
    if (masks_or_null && (st = check_col(g, "ec_sharded_stats", "masks", masks_or_null, n)) != EC_OK) return st;
    for (int i = 0; i < g->n; ++i)
        if ((st = check_stats_cells("ec_sharded_stats", i, t, n[i], "shard it finer")) != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    st = for_each_shard(g, [&](int i) {
        return ec_stats_device(t, p[i], masks_or_null ? masks_or_null[i] : nullptr, n[i], g->payload_dev[i], g->streams[i]);
    });
    const std::string keep = last_error_text();
    const ec_status deferred = take_deferred(g);
    if (deferred != EC_OK) return deferred;
    if (st != EC_OK) return set_error_text(st, keep);
    st = for_each_shard(g, [&](int i) {
        ec_status s = check_hip(hipMemcpyAsync(g->payload_host[i], g->payload_dev[i], sizeof(ec_moments), hipMemcpyDeviceToHost, g->streams[i]),
                                "hipMemcpyAsync(stats record)");
        if (s != EC_OK) return s;
        return check_hip(hipStreamSynchronize(g->streams[i]), "hipStreamSynchronize");
    });
    if (st != EC_OK) return st;
    std::vector<ec_moments> recs(static_cast<size_t>(g->n));
    for (int i = 0; i < g->n; ++i) std::memcpy(&recs[static_cast<size_t>(i)], g->payload_host[i], sizeof(ec_moments));
    return ec_stats_fold(recs.data(), g->n, stats_out);
}

// Zonal statistics of the whole raster, the body of both families' sharded forms: `check` is the family's *_host_args (first on
// no cells: the whole-call refusals of its compute form, n_zones and the types), shard_check(i) refuses shard i's cell count,
// `records` is the family's *_records_host (workspace and records from the shard's pool).  Every shard's n_zones records come
// down, and zone z's records fold in shard order on the host, as ec_sharded_stats' do.  No collective — kind 0 equals the
// unsharded figures bit for bit.
using ZonalHostCheck = ec_status (*)(const char*, ec_dtype, const void*, const uint8_t*, ec_dtype, const void*, size_t, int32_t, const void*);
using ZonalRecordsHost = ec_status (*)(ec_dtype, const void*, const uint8_t*, ec_dtype, const void*, size_t, int32_t, ec_moments*, ec_stream);

template <typename SHARD_CHECK>
static ec_status sharded_zonal(const char* who, ZonalHostCheck check, SHARD_CHECK&& shard_check, ZonalRecordsHost records, ec_shard_group* g, ec_dtype t,
                               const void* const* p, const uint8_t* const* masks_or_null, ec_dtype zt, const void* const* zones, const size_t* n,
                               int32_t n_zones, void* stats_out) {
    ec_status st = check_group(g, who);
    if (st != EC_OK) return st;
    if (!p || !zones || !n || !stats_out) return set_error(EC_ERR_ARG, "%s: null argument", who);
    if ((st = check(who, t, nullptr, nullptr, zt, nullptr, 0, n_zones, stats_out)) != EC_OK) return st;
    if ((st = check_col(g, who, "p", p, n)) != EC_OK) return st;
    if ((st = check_col(g, who, "zones", zones, n)) != EC_OK) return st;
    if (masks_or_null && (st = check_col(g, who, "masks", masks_or_null, n)) != EC_OK) return st;
    for (int i = 0; i < g->n; ++i)
        if ((st = shard_check(i)) != EC_OK) return st;
    std::lock_guard<std::mutex> lk(g->call_mu);
    const size_t nz = static_cast<size_t>(n_zones);
    std::vector<ec_moments> recs(static_cast<size_t>(g->n) * nz);  // shard-major
    st = for_each_shard(g, [&](int i) {
        return records(t, p[i], masks_or_null ? masks_or_null[i] : nullptr, zt, zones[i], n[i], n_zones, &recs[static_cast<size_t>(i) * nz], g->streams[i]);
    });
    const std::string keep = last_error_text();
    const ec_status deferred = take_deferred(g);
    if (deferred != EC_OK) return deferred;
    if (st != EC_OK) return set_error_text(st, keep);
    return fold_zone_records(recs.data(), g->n, nz, stats_out);
}

// ec_zonal_stats_device per shard: up to EC_ZONAL_MAX_ZONES zones.
extern "C" ec_status ec_sharded_zonal_stats(ec_shard_group* g, ec_dtype t, const void* const* p, const uint8_t* const* masks_or_null, ec_dtype zt,
                                            const void* const* zones, const size_t* n, int32_t n_zones, void* stats_out) {
    return sharded_zonal("ec_sharded_zonal_stats", check_zonal_host_args,
                         [&](int i) { return check_stats_cells("ec_sharded_zonal_stats", i, t, n[i], "shard it finer"); }, zonal_records_host, g, t, p,
                         masks_or_null, zt, zones, n, n_zones, stats_out);
}

// ec_zonal_table_device per shard: up to EC_ZONAL_TABLE_MAX_ZONES zones; a shard's cell count against the kind's bound.
extern "C" ec_status ec_sharded_zonal_table(ec_shard_group* g, ec_dtype t, const void* const* p, const uint8_t* const* masks_or_null, ec_dtype zt,
                                            const void* const* zones, const size_t* n, int32_t n_zones, void* stats_out) {
    return sharded_zonal("ec_sharded_zonal_table", check_zonal_table_host_args, [&](int i) {
        return check_zonal_table_host_args("ec_sharded_zonal_table", t, p[i], nullptr, zt, zones[i], n[i], n_zones, stats_out);
    }, zonal_table_records_host, g, t, p, masks_or_null, zt, zones, n, n_zones, stats_out);
}
