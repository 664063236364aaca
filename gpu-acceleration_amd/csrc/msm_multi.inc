// msm_multi.inc -- multi-GPU MSM inside ONE process (include/msm_hip.h "multi-GPU"; SURVEY.md section 8e).  Included by msm_hip.hip.
//
// The reference opens the system default device and nothing else (host/gpu.rs:3-5); behind its signature
// metal_variable_base_msm(&bases, &scalars) (metal_msm.rs:642-695) a caller could never reach a second GPU.  Here one handle
// owns a context per device; a call cuts the point range into contiguous shards, device g's host thread pulls shard g over
// that device's own PCIe link (msm_bn254_g1 on context g: streamed, staged, overlapped exactly as a single-GPU call) and the
// 96-byte partial group elements are exchanged -- there is no data-path collective, MSM is linear in the points.
//
// Exchange.  EC addition is not an RCCL reduction op, so the "all-reduce of partial sums" is an all-gather of 24 words per rank
// followed by a fold in rank order on every rank (identical bits everywhere).  RCCL is reached through dlopen (librccl.so.1 --
// in a PyTorch process that is the copy torch already loaded), so the library has no link-time dependency on it and a box
// without RCCL, a device listed twice, or a single device fall back to the host fold: the partials already sit in host memory
// when the per-device calls return, and the calling thread adds them.
// Types and enums only: every function is resolved with dlsym.  A ROCm install without the RCCL development headers still
// builds the library (and keeps the host fold): the handful of declarations needed are restated here, with the values of
// rccl.h / nccl.h (ncclSuccess = 0; ncclUint32 = 3 in the ncclDataType_t enumeration; ncclComm_t an opaque pointer).
#if defined(__has_include) && __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3 } ncclDataType_t;
#endif

namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // optional
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && AllGather && GetErrorString; }
};
const RcclApi& rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (a.lib) {
            a.CommInitAll = (decltype(a.CommInitAll))dlsym(a.lib, "ncclCommInitAll");
            a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.lib, "ncclCommDestroy");
            a.CommAbort = (decltype(a.CommAbort))dlsym(a.lib, "ncclCommAbort");
            a.AllGather = (decltype(a.AllGather))dlsym(a.lib, "ncclAllGather");
            a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.lib, "ncclGetErrorString");
        }
        return a;
    }();
    return api;
}

thread_local std::string g_multi_create_error;

}  // namespace

struct msm_multi {
    std::mutex mu;
    std::vector<int> dev;
    std::vector<msm_ctx*> ctx;
    HostPool* pool = nullptr;  // ndev - 1 workers; the calling thread drives one device itself
    uint32_t exchange = MSM_MULTI_EXCHANGE_HOST;
    std::string err;
    // RCCL exchange: one communicator, one 24-word send and one 24*ndev-word receive buffer per device, pinned host mirrors
    std::vector<ncclComm_t> comm;
    std::vector<uint32_t*> d_send, d_recv, h_recv;
    // per call
    std::vector<uint32_t> partial;  // ndev x 24 Jacobian Montgomery words
    std::vector<uint32_t> folded;   // ndev x 24: what every rank holds after the RCCL exchange
    std::vector<int32_t> rcs;       // status of every rank's LOCAL MSM ...
    std::vector<int32_t> xrcs;      // ... and of its part of the exchange
    // rendezvous in front of the collective: ranks whose local MSM has returned, guarded by rv_mu; a rank BLOCKS here (condition
    // variable, no spinning: the fast ranks' cores belong to the finish threads of the ranks still running) and gives up after
    // rendezvous_timeout_s, naming the ranks that never came
    std::mutex rv_mu;
    std::condition_variable rv_cv;
    int arrived = 0;
    uint64_t rv_gen = 0;            // call generation: a rank that arrives after its call was abandoned must not enter a collective alone
    bool rv_abandoned = false;      // this call's rendezvous timed out on some rank: nobody enters the collective
    double rendezvous_timeout_s = 600.0;  // MSM_HIP_MULTI_TIMEOUT_S at creation
    bool broken = false;            // a collective failed or a rank never reached the rendezvous: the communicators are unusable
    bool verify_ranks = false;      // MSM_HIP_MULTI_VERIFY=1 at creation: compare every rank's folded bits after the all-gather
    // statistics of the last call (msm_multi_get_exchange_stats): wall clock of each rank's local MSM and of rank 0's exchange
    std::vector<float> shard_ms;
    float exchange_ms = 0;
    // AUTO on more than one distinct device: what msm_multi_create measured for the two exchanges (ms per call on identity partials, no
    // MSM in front: the exchange alone), 0 = not probed (msm_multi_get_exchange_probe)
    float probe_rccl_ms = 0, probe_host_ms = 0;
};

namespace {

int32_t mfail(msm_multi* m, int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (m) m->err = buf;
    else g_multi_create_error = buf;
    return code;
}

void multi_release(msm_multi* m) {
    if (!m) return;
    delete m->pool;
    for (size_t g = 0; g < m->ctx.size(); g++) {
        if (g < m->dev.size()) (void)hipSetDevice(m->dev[g]);
        if (g < m->comm.size() && m->comm[g]) (void)rccl_api().CommDestroy(m->comm[g]);
        if (g < m->d_send.size() && m->d_send[g]) (void)hipFree(m->d_send[g]);
        if (g < m->d_recv.size() && m->d_recv[g]) (void)hipFree(m->d_recv[g]);
        if (g < m->h_recv.size() && m->h_recv[g]) (void)hipHostFree(m->h_recv[g]);
        msm_ctx_destroy(m->ctx[g]);
    }
    delete m;
}

// exchange + fold for rank g after its local MSM: partial g -> HBM -> all-gather -> pinned host -> fold in rank order.
// Entered by ALL ranks or by none (multi_run).  Once inside, a rank joins the collective even when the 96-byte upload in front of
// it failed -- its peers are already waiting -- and reports the error afterwards.
int32_t rccl_exchange(msm_multi* m, int g) {
    const int G = (int)m->ctx.size();
    msm_ctx* c = m->ctx[(size_t)g];
    hipStream_t st = c->stream;
    DeviceGuard dg(m->dev[(size_t)g]);  // (the caller's thread drives one rank itself: its current device is restored)
    hipError_t e = dg.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_send[(size_t)g], &m->partial[(size_t)g * 24], 96, hipMemcpyHostToDevice, st);
    ncclResult_t r = rccl_api().AllGather(m->d_send[(size_t)g], m->d_recv[(size_t)g], 24, ncclUint32, m->comm[(size_t)g], st);
    if (r != ncclSuccess) {
        // This rank's part of the collective was not enqueued: its peers' all-gather cannot complete.  Drain what this rank did queue,
        // abort the communicator so that the peers' collective ends with an error instead of waiting (ncclCommAbort, when the library
        // has it), and mark the handle unusable: every later call returns MSM_ERR_RCCL until it is destroyed and created again.
        (void)hipStreamSynchronize(st);
        if (rccl_api().CommAbort) {
            (void)rccl_api().CommAbort(m->comm[(size_t)g]);
            m->comm[(size_t)g] = nullptr;
        }
        {
            std::lock_guard<std::mutex> lk(m->rv_mu);
            m->broken = true;
        }
        c->err = std::string("ncclAllGather failed: ") + rccl_api().GetErrorString(r);
        return MSM_ERR_RCCL;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(m->h_recv[(size_t)g], m->d_recv[(size_t)g], (size_t)96 * G, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        c->err = std::string("exchange copy failed: ") + hipGetErrorString(e);
        return MSM_ERR_HIP;
    }
    return msm_bn254_g1_combine(m->h_recv[(size_t)g], (size_t)G, &m->folded[(size_t)g * 24], nullptr, nullptr);
}

// run `local(g, out_jac24)` for every device on its own host thread, exchange, fold.
//
// NO RANK MAY HANG (the reference returns Err, metal_msm.rs:647-656; here: a status code on every path).  A rank whose local MSM
// fails -- one scalar >= 2^254 in its shard is enough -- must not leave its peers waiting in ncclAllGather for a partner that never
// comes.  The ranks are host threads of one process, so the status "all-gather" costs nothing: every rank publishes the status of its
// local MSM and waits at a rendezvous until all have; only if EVERY local MSM succeeded does anyone enter the collective.  Otherwise all
// ranks skip it and the call returns the first failing rank's code and message.
template <class F>
int32_t multi_run(msm_multi* m, const std::vector<size_t>& cnt, F&& local, uint32_t* out_jac, uint32_t* out_aff, uint8_t* out_inf) {
    Range r_("msm_multi");
    const int G = (int)m->ctx.size();
    static const hostg1::Jac ident = hostg1::identity();
    std::fill(m->rcs.begin(), m->rcs.end(), MSM_OK);
    std::fill(m->xrcs.begin(), m->xrcs.end(), MSM_OK);
    m->exchange_ms = 0;
    const bool use_rccl = m->exchange == MSM_MULTI_EXCHANGE_RCCL;  // (needs one host thread per rank: msm_multi_create guarantees the pool)
    const bool canonical = !m->ctx.empty() && (m->ctx[0]->cfg.flags & MSM_FLAG_DETERMINISTIC) != 0;  // every per-device context carries cfg->flags
    uint64_t my_gen;
    {
        std::lock_guard<std::mutex> lk(m->rv_mu);
        if (m->broken)
            return mfail(m, MSM_ERR_RCCL, "this handle's RCCL communicators are unusable after a failed collective or a rank that never "
                                          "reached the rendezvous: destroy it and create a new one");
        m->arrived = 0;
        m->rv_abandoned = false;
        my_gen = ++m->rv_gen;
    }
    std::vector<char> at_rv((size_t)G, 0);  // which ranks reached the rendezvous (guarded by rv_mu): names the missing ones on a timeout
    auto job = [&](int g) {
        uint32_t* part = &m->partial[(size_t)g * 24];
        const auto t0 = std::chrono::steady_clock::now();
        int32_t rc = MSM_OK;
        if (cnt[(size_t)g] == 0) hostg1::store_jac(part, ident);  // more devices than points: this rank contributes the identity
        else rc = local(g, part);
        if (rc != MSM_OK) hostg1::store_jac(part, ident);
        m->rcs[(size_t)g] = rc;
        const auto t1 = std::chrono::steady_clock::now();
        m->shard_ms[(size_t)g] = std::chrono::duration<float, std::milli>(t1 - t0).count();
        if (!use_rccl) return;
        {
            std::unique_lock<std::mutex> lk(m->rv_mu);
            if (m->rv_gen != my_gen) return;  // (cannot happen while multi_run holds the handle's mutex; kept as a guard)
            at_rv[(size_t)g] = 1;
            if (++m->arrived == G) {
                m->rv_cv.notify_all();
            } else {
                const bool all = m->rv_cv.wait_for(lk, std::chrono::duration<double>(m->rendezvous_timeout_s),
                                                   [&] { return m->arrived == G || m->rv_abandoned; });
                if (!all && !m->rv_abandoned) {  // first rank to give up: the call is abandoned for everyone, the handle is done
                    m->rv_abandoned = true;
                    m->broken = true;
                    std::string missing;
                    for (int k = 0; k < G; k++)
                        if (!at_rv[(size_t)k]) missing += (missing.empty() ? "" : ", ") + std::to_string(k);
                    m->ctx[(size_t)g]->err = "rank(s) " + missing + " did not reach the rendezvous in front of the all-gather within " +
                                             std::to_string((int)m->rendezvous_timeout_s) + " s";
                    m->xrcs[(size_t)g] = MSM_ERR_HIP;
                    m->rv_cv.notify_all();
                }
            }
            if (m->rv_abandoned) return;  // nobody enters the collective; a rank that arrives late finds the flag and leaves too
        }
        for (int k = 0; k < G; k++)
            if (m->rcs[(size_t)k] != MSM_OK) return;  // every rank reads the same G words: all skip the collective together
        m->xrcs[(size_t)g] = rccl_exchange(m, g);
        if (g == 0) m->exchange_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
    };
    if (m->pool && G > 1) m->pool->run(G, job);
    else
        for (int g = 0; g < G; g++) job(g);  // G == 1, or host fold without a pool
    for (int g = 0; g < G; g++)
        if (m->rcs[(size_t)g] != MSM_OK)
            return mfail(m, m->rcs[(size_t)g], "device %d (rank %d): %s", m->dev[(size_t)g], g, msm_last_error(m->ctx[(size_t)g]));
    for (int g = 0; g < G; g++)
        if (m->xrcs[(size_t)g] != MSM_OK)
            return mfail(m, m->xrcs[(size_t)g], "exchange on device %d (rank %d): %s", m->dev[(size_t)g], g, msm_last_error(m->ctx[(size_t)g]));
    if (use_rccl && m->rv_abandoned) return mfail(m, MSM_ERR_HIP, "the rendezvous in front of the all-gather was abandoned");
    if (use_rccl) {
        if (m->verify_ranks)  // debug: every rank folded the same 24*G words in the same order
            for (int g = 1; g < G; g++)
                if (std::memcmp(&m->folded[0], &m->folded[(size_t)g * 24], 96) != 0)
                    return mfail(m, MSM_ERR_RCCL, "rank %d holds a different result than rank 0 after the all-gather", g);
        return combine_partials<HostG1>(&m->folded[0], 1, out_jac, out_aff, out_inf, canonical);
    }
    const auto tx = std::chrono::steady_clock::now();
    const int32_t rc = combine_partials<HostG1>(m->partial.data(), (size_t)G, out_jac, out_aff, out_inf, canonical);  // host fold, rank order
    m->exchange_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tx).count();
    return rc;
}

std::vector<size_t> shard_bounds(size_t n, int G) {
    std::vector<size_t> lo((size_t)G + 1);
    for (int g = 0; g <= G; g++) lo[(size_t)g] = (size_t)((unsigned __int128)n * (unsigned)g / (unsigned)G);
    return lo;
}

}  // namespace

extern "C" {

const char* msm_multi_last_error(const msm_multi* m) { return m ? m->err.c_str() : g_multi_create_error.c_str(); }
int32_t msm_multi_num_devices(const msm_multi* m) { return m ? (int32_t)m->ctx.size() : 0; }
uint32_t msm_multi_exchange(const msm_multi* m) { return m ? m->exchange : 0u; }

int32_t msm_multi_create(const int32_t* devices, int32_t ndev, const msm_config_t* cfg, uint32_t exchange, msm_multi** out) {
    if (!out) return mfail(nullptr, MSM_ERR_BAD_ARG, "out == NULL");
    *out = nullptr;
    if (exchange > MSM_MULTI_EXCHANGE_HOST) return mfail(nullptr, MSM_ERR_BAD_ARG, "unknown exchange mode %u", exchange);
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible == 0)
        return mfail(nullptr, MSM_ERR_NO_DEVICE, "no HIP device visible: this engine has no CPU fallback");
    struct RestoreDevice {  // the setup below visits every device; the caller's current device is what it was when this function returns
        int prev = -1;
        RestoreDevice() {
            if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        }
        ~RestoreDevice() {
            if (prev >= 0) (void)hipSetDevice(prev);
        }
    } restore_device;
    std::vector<int> dev;
    if (devices) {
        if (ndev <= 0 || ndev > 64) return mfail(nullptr, MSM_ERR_BAD_ARG, "ndev = %d out of range [1, 64]", ndev);
        dev.assign(devices, devices + ndev);
    } else if (const char* e = std::getenv("MSM_HIP_DEVICES")) {
        for (const char* p = e; *p;) {
            char* end = nullptr;
            long v = std::strtol(p, &end, 10);
            if (end == p) break;
            dev.push_back((int)v);
            p = *end == ',' ? end + 1 : end;
        }
        if (dev.empty()) return mfail(nullptr, MSM_ERR_BAD_ARG, "MSM_HIP_DEVICES=\"%s\" names no device", e);
    } else {
        for (int d = 0; d < visible; d++) dev.push_back(d);
    }
    bool dup = false;
    for (size_t i = 0; i < dev.size(); i++) {
        if (dev[i] < 0 || dev[i] >= visible) return mfail(nullptr, MSM_ERR_NO_DEVICE, "device %d out of range (%d visible)", dev[i], visible);
        for (size_t j = 0; j < i; j++) dup = dup || dev[j] == dev[i];
    }
    const int G = (int)dev.size();
    msm_multi* m = new (std::nothrow) msm_multi();
    if (!m) return mfail(nullptr, MSM_ERR_OOM, "host allocation failed");
    m->dev = dev;
    msm_config_t c0{};
    if (cfg) c0 = *cfg;
    for (int g = 0; g < G; g++) {
        c0.device = dev[(size_t)g];
        msm_ctx* c = nullptr;
        int32_t rc = msm_ctx_create(&c0, &c);
        if (rc) {
            mfail(nullptr, rc, "context on device %d: %s", dev[(size_t)g], msm_last_error(nullptr));
            multi_release(m);
            return rc;
        }
        c->no_host_pin = true;  // the handle pins the caller's arrays once for all its ranks
        m->ctx.push_back(c);
    }
    m->partial.assign((size_t)G * 24, 0u);
    m->folded.assign((size_t)G * 24, 0u);
    m->rcs.assign((size_t)G, MSM_OK);
    m->xrcs.assign((size_t)G, MSM_OK);
    m->shard_ms.assign((size_t)G, 0.f);
#ifdef MSM_HIP_TEST_HOOKS
    if (const char* e = std::getenv("MSM_HIP_MULTI_VERIFY")) m->verify_ranks = *e && *e != '0';  // (debug knob of the hooks build)
#endif
    if (const char* e = std::getenv("MSM_HIP_MULTI_TIMEOUT_S")) {
        const double v = std::atof(e);
        if (v > 0) m->rendezvous_timeout_s = std::min(v, 30.0 * 86400.0);  // (clamped: wait_for converts to nanoseconds, 1e12 s would overflow)
    }
    if (G > 1) {
        m->pool = new (std::nothrow) HostPool(G - 1);  // one host thread per rank: the ranks rendezvous in front of the collective
        if (!m->pool) {
            mfail(nullptr, MSM_ERR_OOM, "host allocation failed");
            multi_release(m);
            return MSM_ERR_OOM;
        }
    }
    // exchange mode
    const bool rccl_possible = rccl_api().ok() && !dup && (G > 1 || exchange == MSM_MULTI_EXCHANGE_RCCL);
    if (exchange == MSM_MULTI_EXCHANGE_RCCL && !rccl_possible) {
        mfail(nullptr, MSM_ERR_RCCL, dup ? "RCCL exchange needs distinct devices" : "librccl could not be loaded: %s", dlerror());
        multi_release(m);
        return MSM_ERR_RCCL;
    }
    if (exchange != MSM_MULTI_EXCHANGE_HOST && rccl_possible) {
        m->comm.assign((size_t)G, nullptr);
        m->d_send.assign((size_t)G, nullptr);
        m->d_recv.assign((size_t)G, nullptr);
        m->h_recv.assign((size_t)G, nullptr);
        ncclResult_t r = rccl_api().CommInitAll(m->comm.data(), G, m->dev.data());
        hipError_t e = hipSuccess;
        for (int g = 0; g < G && r == ncclSuccess && e == hipSuccess; g++) {
            e = hipSetDevice(dev[(size_t)g]);
            if (e == hipSuccess) e = hipMalloc((void**)&m->d_send[(size_t)g], 96);
            if (e == hipSuccess) e = hipMalloc((void**)&m->d_recv[(size_t)g], (size_t)96 * G);
            if (e == hipSuccess) e = hipHostMalloc((void**)&m->h_recv[(size_t)g], (size_t)96 * G, hipHostMallocDefault);
        }
        if (r != ncclSuccess || e != hipSuccess) {
            if (exchange == MSM_MULTI_EXCHANGE_RCCL) {
                mfail(nullptr, r != ncclSuccess ? MSM_ERR_RCCL : MSM_ERR_HIP, "RCCL exchange setup failed: %s",
                      r != ncclSuccess ? rccl_api().GetErrorString(r) : hipGetErrorString(e));
                multi_release(m);
                return r != ncclSuccess ? MSM_ERR_RCCL : MSM_ERR_HIP;
            }
            // AUTO: quietly keep the host fold (the communicators that did come up are released with the handle)
        } else {
            m->exchange = MSM_MULTI_EXCHANGE_RCCL;
        }
    }
    // AUTO decides by MEASUREMENT, once, here (round 5; VERDICT r4 item 4).  Each rank's partial already sits in host memory when its
    // local call returns (the Horner finish runs on the CPU), so the RCCL exchange -- 96 B up, ncclAllGather, 96 * G B down, a stream
    // synchronisation, the fold on every rank -- is by construction MORE work than the calling thread folding G partials; rounds 2-4
    // preferred it unmeasured.  Both exchanges run a few times on identity partials (no MSM in front: the exchange alone, the same code
    // path the calls take) and the faster one stays for the handle's life; an explicit MSM_MULTI_EXCHANGE_RCCL / _HOST is never probed.
    if (exchange == MSM_MULTI_EXCHANGE_AUTO && m->exchange == MSM_MULTI_EXCHANGE_RCCL) {
        const std::vector<size_t> none((size_t)G, 0);  // every rank contributes the identity
        auto nothing = [](int, uint32_t*) { return (int32_t)MSM_OK; };
        float best[2] = {0, 0};
        bool rccl_ok = true;
        for (int mode = 0; mode < 2 && rccl_ok; mode++) {
            m->exchange = mode == 0 ? MSM_MULTI_EXCHANGE_RCCL : MSM_MULTI_EXCHANGE_HOST;
            for (int rep = 0; rep < 6; rep++) {  // the first call of a communicator sets its channels up: it is run, not counted
                const auto t0 = std::chrono::steady_clock::now();
                const int32_t rc = multi_run(m, none, nothing, nullptr, nullptr, nullptr);
                const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (rc != MSM_OK) {
                    rccl_ok = rccl_ok && mode == 1;
                    break;
                }
                if (rep > 0 && (best[mode] == 0 || ms < best[mode])) best[mode] = ms;
            }
        }
        m->probe_rccl_ms = best[0], m->probe_host_ms = best[1];
        if (!rccl_ok) {  // the collective failed on its first use: the host fold needs no communicator
            std::lock_guard<std::mutex> lk(m->rv_mu);
            m->broken = false;
            m->exchange = MSM_MULTI_EXCHANGE_HOST;
        } else {
            m->exchange = best[0] > 0 && best[0] < best[1] ? MSM_MULTI_EXCHANGE_RCCL : MSM_MULTI_EXCHANGE_HOST;
        }
        m->err.clear();
    }
    *out = m;
    return MSM_OK;
}
int32_t msm_multi_get_exchange_probe(const msm_multi* m, float* rccl_ms, float* host_ms) {
    if (!m) return MSM_ERR_BAD_ARG;
    if (rccl_ms) *rccl_ms = m->probe_rccl_ms;
    if (host_ms) *host_ms = m->probe_host_ms;
    return MSM_OK;
}

void msm_multi_destroy(msm_multi* m) {
    if (!m) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    multi_release(m);
    if (prev >= 0) (void)hipSetDevice(prev);
}

int32_t msm_bn254_g1_multi(msm_multi* m, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask,
                           const uint32_t* scalars, size_t n, uint32_t out_jac[24], uint32_t out_aff[16], uint8_t* out_inf) {
    if (!m) return MSM_ERR_BAD_ARG;
    if (n == 0) return mfail(m, MSM_ERR_EMPTY, "Empty input");  // metal_msm.rs:647-649
    if (!bases_xy || !scalars) return mfail(m, MSM_ERR_BAD_ARG, "NULL bases/scalars pointer");
    std::lock_guard<std::mutex> lk(m->mu);
    const int G = (int)m->ctx.size();
    const std::vector<size_t> lo = shard_bounds(n, G);
    std::vector<size_t> cnt((size_t)G);
    for (int g = 0; g < G; g++) cnt[(size_t)g] = lo[(size_t)g + 1] - lo[(size_t)g];
    HostPin pin_b, pin_s, pin_i;  // ONE registration of the caller's arrays for all ranks (the ranks' own would overlap at the shard borders' pages)
    pin_b.pin(bases_xy, n * 64, true);
    pin_s.pin(scalars, n * 32, true);
    pin_i.pin(inf_mask, n, true);
    return multi_run(
        m, cnt,
        [&](int g, uint32_t* part) {
            const size_t a = lo[(size_t)g];
            return msm_bn254_g1(m->ctx[(size_t)g], bases_xy + a * 16, base_form, inf_mask ? inf_mask + a : nullptr, scalars + a * 8,
                                cnt[(size_t)g], part, nullptr, nullptr);
        },
        out_jac, out_aff, out_inf);
}

int32_t msm_bn254_g1_multi_arkworks(msm_multi* m, const void* bases, size_t stride, size_t x_off, size_t y_off, size_t inf_off,
                                    const uint32_t* scalars_mont, size_t n, uint32_t out_jac[24], uint32_t out_aff[16],
                                    uint8_t* out_inf) {
    if (!m) return MSM_ERR_BAD_ARG;
    if (n == 0) return mfail(m, MSM_ERR_EMPTY, "Empty input");
    if (!bases || !scalars_mont) return mfail(m, MSM_ERR_BAD_ARG, "NULL bases/scalars pointer");
    std::lock_guard<std::mutex> lk(m->mu);
    const int G = (int)m->ctx.size();
    const std::vector<size_t> lo = shard_bounds(n, G);
    std::vector<size_t> cnt((size_t)G);
    for (int g = 0; g < G; g++) cnt[(size_t)g] = lo[(size_t)g + 1] - lo[(size_t)g];
    HostPin pin_b, pin_s;
    pin_b.pin(bases, n * stride, true);
    pin_s.pin(scalars_mont, n * 32, true);
    return multi_run(
        m, cnt,
        [&](int g, uint32_t* part) {
            const size_t a = lo[(size_t)g];
            return msm_bn254_g1_arkworks(m->ctx[(size_t)g], (const uint8_t*)bases + a * stride, stride, x_off, y_off, inf_off,
                                         scalars_mont + a * 8, cnt[(size_t)g], part, nullptr, nullptr);
        },
        out_jac, out_aff, out_inf);
}

int32_t msm_bn254_g1_multi_device(msm_multi* m, const void* const* d_bases_mont, const void* const* d_inf_masks,
                                  const void* const* d_scalars, const size_t* n_per_dev, uint32_t out_jac[24], uint32_t out_aff[16],
                                  uint8_t* out_inf) {
    if (!m) return MSM_ERR_BAD_ARG;
    if (!d_bases_mont || !d_scalars || !n_per_dev) return mfail(m, MSM_ERR_BAD_ARG, "NULL pointer array");
    std::lock_guard<std::mutex> lk(m->mu);
    const int G = (int)m->ctx.size();
    std::vector<size_t> cnt(n_per_dev, n_per_dev + G);
    size_t total = 0;
    for (int g = 0; g < G; g++) total += cnt[(size_t)g];
    if (total == 0) return mfail(m, MSM_ERR_EMPTY, "Empty input");
    return multi_run(
        m, cnt,
        [&](int g, uint32_t* part) {
            return msm_bn254_g1_device(m->ctx[(size_t)g], d_bases_mont[g], d_inf_masks ? d_inf_masks[g] : nullptr, d_scalars[g],
                                       cnt[(size_t)g], nullptr, part, nullptr, nullptr);
        },
        out_jac, out_aff, out_inf);
}

int32_t msm_multi_get_exchange_stats(const msm_multi* m, float* exchange_ms, float* shard_ms, int32_t nshard) {
    if (!m) return MSM_ERR_BAD_ARG;
    if (exchange_ms) *exchange_ms = m->exchange_ms;
    if (shard_ms)
        for (int32_t g = 0; g < nshard && g < (int32_t)m->shard_ms.size(); g++) shard_ms[g] = m->shard_ms[(size_t)g];
    return MSM_OK;
}

int32_t msm_multi_get_timings(const msm_multi* m, int32_t g, msm_timings_t* out) {
    if (!m || !out || g < 0 || g >= (int32_t)m->ctx.size()) return MSM_ERR_BAD_ARG;
    return msm_get_timings(m->ctx[(size_t)g], out);
}
int32_t msm_multi_set_kernel_timing(msm_multi* m, uint32_t every_n) {
    if (!m) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    for (msm_ctx* c : m->ctx) {
        const int32_t rc = msm_set_kernel_timing(c, every_n);
        if (rc) return rc;
    }
    return MSM_OK;
}
int32_t msm_multi_get_clock_stats(msm_multi* m, int32_t g, double* sclk_ghz, double* cycles_per_addition, uint64_t* samples) {
    if (!m || g < 0 || g >= (int32_t)m->ctx.size()) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    return msm_get_clock_stats(m->ctx[(size_t)g], sclk_ghz, cycles_per_addition, samples);
}
int32_t msm_multi_get_timings_sized(const msm_multi* m, int32_t g, void* out, size_t out_size) {
    if (!m || !out || g < 0 || g >= (int32_t)m->ctx.size()) return MSM_ERR_BAD_ARG;
    return msm_get_timings_sized(m->ctx[(size_t)g], out, out_size);
}

}  // extern "C"
