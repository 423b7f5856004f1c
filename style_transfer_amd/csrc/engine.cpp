// libstx host side: the tile engine behind include/stx.h.
//
// One engine = one GPU + one HIP stream + one copy of the network (graph, weights packed for the
// MFMA kernels) + the current targets (content feature maps, style Grams).  It plays the role of
// the reference's TileWorker process (style_transfer.py:169-259) with CaffeModel.eval_features_tile
// / eval_sc_grad_tile (style_transfer.py:421-427,556-612) inside, but is driven by plain function
// calls that enqueue kernels asynchronously instead of pickled messages over multiprocessing
// queues and POSIX shared memory.
//
// This file: the engine's life cycle and weights, the scalar arenas and their fences, and the profiling
// readers.  engine.h says which host file owns what.

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "engine.h"

namespace stx {

static thread_local std::string g_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

int alloc_scalars(stx_engine *e, size_t n, size_t *index) {
    stx_engine::ScalarArena &a = e->A();
    if (a.used + n > e->scalars_cap) {
        set_error("scalar arena exhausted (%zu + %zu > %zu)", a.used, n, e->scalars_cap);
        return STX_ERR_NOMEM;
    }
    *index = a.used;
    a.used += n;
    return STX_OK;
}

int alloc_dscalars(stx_engine *e, size_t n, size_t *index) {
    stx_engine::ScalarArena &a = e->A();
    if (a.dused + n > e->dscalars_cap - 4) {   // the last slots serve synchronous results
        // no wrap: results are consumed at every stx_sync / stx_fence_wait, which also resets the arena
        set_error("double-scalar arena exhausted; call stx_sync more often");
        return STX_ERR_NOMEM;
    }
    *index = a.dused;
    a.dused += n;
    return STX_OK;
}

// Copies caller memory (host or device) into a device destination on the engine stream.
int copy_in(stx_engine *e, void *dst, const void *src, int mem, size_t bytes) {
    if (mem == STX_HOST)
        STX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
    else   // the source may live on another GPU of the node (peer copy over xGMI)
        STX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
    return STX_OK;
}

int copy_out(stx_engine *e, void *dst, int mem, const void *src, size_t bytes) {
    if (mem == STX_HOST)
        STX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
    else
        STX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
    return STX_OK;
}

// Publishes the losses of one arena from its host mirrors (the copies have landed) and empties it.
static void publish_arena(stx_engine::ScalarArena &a) {
    for (const PendingLoss &pl : a.pending) {
        double v = 0.0;
        for (const LossTerm &t : pl.terms) v += t.coef * (double)a.host[t.scalar_index];
        for (const LossTerm &t : pl.dterms) v += t.coef * a.dhost[t.scalar_index];
        if (pl.out) *pl.out = v;
    }
    a.pending.clear();
    a.used = 0;
    a.dused = 0;
    a.ticket = 0;
}

int do_sync(stx_engine *e) {
    STX_HIP(hipStreamSynchronize(e->stream));
    e->flow_work.release();     // (the flow estimator's workspace, about 300 B per pixel: its launches are done)
    e->poisson_work.release();  // (the screened-Poisson stage's, 64 B per pixel)
    // the closed arena (if any) is the older one
    publish_arena(e->arena[e->cur ^ 1]);
    publish_arena(e->arena[e->cur]);
    return STX_OK;
}

// Waits for the streams of every engine that shares e's state (weights or targets are about to be
// replaced under them).  Their pending results stay pending.
int quiesce_members(stx_engine *e) {
    for (stx_engine *m : e->sh->members) STX_HIP(hipStreamSynchronize(m->stream));
    return STX_OK;
}

// ---- the switches' snapshot (common.h: sw_env).  Old snapshots are never freed: a thread may still hold a
// pointer into one, and a snapshot is a few hundred bytes.
namespace {
typedef std::map<std::string, std::string> SwitchMap;
std::atomic<const SwitchMap *> g_switches{nullptr};
std::mutex g_switches_mutex;
extern "C" char **environ;

const SwitchMap *switches_snapshot() {
    auto *m = new SwitchMap;
    for (char **e = environ; e && *e; ++e) {
        if (strncmp(*e, "STX_", 4) != 0) continue;
        const char *eq = strchr(*e, '=');
        if (eq) (*m)[std::string(*e, eq - *e)] = eq + 1;
    }
    return m;
}
}  // namespace

void sw_reread() {
    std::lock_guard<std::mutex> lock(g_switches_mutex);
    g_switches.store(switches_snapshot(), std::memory_order_release);
}

const char *sw_env(const char *name) {
    const SwitchMap *m = g_switches.load(std::memory_order_acquire);
    if (!m) {
        std::lock_guard<std::mutex> lock(g_switches_mutex);
        m = g_switches.load(std::memory_order_acquire);
        if (!m) {
            m = switches_snapshot();
            g_switches.store(m, std::memory_order_release);
        }
    }
    auto it = m->find(name);
    return it == m->end() ? nullptr : it->second.c_str();
}
}  // namespace stx

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char *stx_version(void) { return "libstx 0.1 (gfx950)"; }

int stx_reread_env(void) {
    stx::sw_reread();
    return STX_OK;
}

const char *stx_last_error(void) { return g_error.c_str(); }

int stx_device_count(int *count) {
    if (!count) return STX_ERR_ARG;
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return STX_OK;
}

int stx_device_name(int device, char *buf, size_t buf_len) {
    if (!buf || !buf_len) return STX_ERR_ARG;
    hipDeviceProp_t prop;
    STX_HIP(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buf_len, "%s", prop.gcnArchName);
    return STX_OK;
}

}  // extern "C"

// Peer access between the GPUs of the node (tile and target copies of a multi-GPU farm are peer
// reads / writes over xGMI).  Tried once per device; a pair that cannot be enabled is remembered
// and reported once on stderr -- copies between those two GPUs still work (the runtime stages
// them through host memory), they are only slower.  STX_Q_PEERS_WITHOUT_ACCESS counts them.
static std::mutex g_peer_mutex;
static std::map<int, std::vector<int>> g_peers_missing;   // device -> peers without direct access

void enable_peer_access(int device) {
    std::lock_guard<std::mutex> lock(g_peer_mutex);
    if (g_peers_missing.count(device)) return;
    std::vector<int> &missing = g_peers_missing[device];
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    for (int peer = 0; peer < n_dev; ++peer) {
        if (peer == device) continue;
        int can = 0;
        hipError_t err = hipDeviceCanAccessPeer(&can, device, peer);
        if (err == hipSuccess && can) {
            err = hipDeviceEnablePeerAccess(peer, 0);
            if (err == hipErrorPeerAccessAlreadyEnabled) err = hipSuccess;
        } else if (err == hipSuccess) {
            err = hipErrorPeerAccessUnsupported;
        }
        (void)hipGetLastError();
        if (err != hipSuccess) {
            missing.push_back(peer);
            fprintf(stderr, "libstx: no peer access GPU %d -> GPU %d (%s); copies between them are "
                            "staged by the runtime\n", device, peer, hipGetErrorString(err));
        }
    }
}

int peers_without_access(int device) {
    std::lock_guard<std::mutex> lock(g_peer_mutex);
    auto it = g_peers_missing.find(device);
    return it == g_peers_missing.end() ? 0 : (int)it->second.size();
}

constexpr size_t kScalarFloats = 1 << 18;   // per-call scalar arena (sums + small partials)

// `share`: the state of an engine on the same GPU to join (weights, packed banks, targets), or null.
static int build_engine(int device, const stx_layer_desc *layers, int n_layers,
                        std::shared_ptr<SharedState> share, stx_engine **out) {
    if (!layers || n_layers < 2 || !out) {
        set_error("stx_engine_create: bad arguments");
        return STX_ERR_ARG;
    }
    if (layers[0].type != STX_LAYER_INPUT || !layers[0].top) {
        set_error("stx_engine_create: layer 0 must be the input layer");
        return STX_ERR_ARG;
    }
    std::unique_ptr<stx_engine> e(new stx_engine);
    e->device = device;
    const bool joined = share != nullptr;
    e->sh = joined ? share : std::make_shared<SharedState>();
    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        set_error("hipSetDevice(%d): %s", device, hipGetErrorString(err));
        return STX_ERR_HIP;
    }
    auto add_blob = [&](const std::string &name, int channels, int producer) {
        Blob b;
        b.name = name;
        b.channels = channels;
        b.producer = producer;
        e->blob_index[name] = (int)e->blobs.size();
        e->blobs.push_back(std::move(b));
        return (int)e->blobs.size() - 1;
    };
    for (int i = 0; i < n_layers; ++i) {
        const stx_layer_desc &d = layers[i];
        Layer L;
        L.name = d.name ? d.name : "";
        L.bottom = d.bottom ? d.bottom : "";
        L.top = d.top ? d.top : "";
        L.type = d.type;
        L.num_output = d.num_output;
        L.ksize = d.kernel_size;
        L.pad = d.pad;
        L.stride = d.stride;
        L.pool_mode = d.pool_mode;
        if (L.top.empty()) {
            set_error("layer %d (%s) has no top blob", i, L.name.c_str());
            return STX_ERR_ARG;
        }
        if (i == 0) {
            L.top_blob = add_blob(L.top, d.num_output > 0 ? d.num_output : 3, 0);
        } else {
            auto it = e->blob_index.find(L.bottom);
            if (it == e->blob_index.end()) {
                set_error("layer %s: unknown bottom blob '%s'", L.name.c_str(), L.bottom.c_str());
                return STX_ERR_ARG;
            }
            L.bottom_blob = it->second;
            if (L.type == STX_LAYER_RELU) {
                if (L.top != L.bottom) {
                    set_error("layer %s: only in-place ReLU is supported", L.name.c_str());
                    return STX_ERR_UNSUPPORTED;
                }
                L.top_blob = L.bottom_blob;
                e->blobs[L.top_blob].relu = true;
            } else if (L.type == STX_LAYER_CONV) {
                if (!((L.ksize == 3 && L.pad == 1) || (L.ksize == 1 && L.pad == 0))) {
                    set_error("layer %s: only 3x3/pad 1 and 1x1/pad 0 convolutions are supported",
                              L.name.c_str());
                    return STX_ERR_UNSUPPORTED;
                }
                if (e->blob_index.count(L.top)) {
                    set_error("layer %s: top blob '%s' already exists", L.name.c_str(), L.top.c_str());
                    return STX_ERR_UNSUPPORTED;
                }
                L.top_blob = add_blob(L.top, L.num_output, i);
                if (!joined) {
                    ConvParams &cp = e->sh->conv[i];
                    cp.cin = e->blobs[L.bottom_blob].channels;
                    cp.cout = L.num_output;
                    cp.ks = L.ksize;
                }
            } else if (L.type == STX_LAYER_POOL) {
                if (L.ksize != 2 || L.stride != 2 ||
                    (L.pool_mode != STX_POOL_MAX && L.pool_mode != STX_POOL_AVE)) {
                    set_error("layer %s: only 2x2 stride-2 MAX/AVE pooling is supported",
                              L.name.c_str());
                    return STX_ERR_UNSUPPORTED;
                }
                if (e->blob_index.count(L.top)) {
                    set_error("layer %s: top blob '%s' already exists", L.name.c_str(), L.top.c_str());
                    return STX_ERR_UNSUPPORTED;
                }
                L.top_blob = add_blob(L.top, e->blobs[L.bottom_blob].channels, i);
            } else {
                set_error("layer %s: unsupported type %d", L.name.c_str(), L.type);
                return STX_ERR_UNSUPPORTED;
            }
        }
        e->layer_index[L.name] = i;
        e->layers.push_back(std::move(L));
    }
    // scale of every blob: 224 // (blob height for a 224 x 224 input)
    {
        std::vector<int> h224(e->blobs.size(), 224);
        for (size_t li = 1; li < e->layers.size(); ++li) {
            const Layer &L = e->layers[li];
            if (L.type == STX_LAYER_CONV) h224[L.top_blob] = h224[L.bottom_blob];
            if (L.type == STX_LAYER_POOL) h224[L.top_blob] = pooled_len(h224[L.bottom_blob]);
        }
        for (size_t bi = 0; bi < e->blobs.size(); ++bi) e->blobs[bi].scale = 224 / h224[bi];
    }
    enable_peer_access(device);
    STX_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    for (int i = 0; i < stx_engine::kTimed; ++i) {
        STX_HIP(hipEventCreate(&e->ev_start[i]));
        STX_HIP(hipEventCreate(&e->ev_stop[i]));
    }
    STX_HIP(hipEventCreate(&e->ev_tune0));
    STX_HIP(hipEventCreate(&e->ev_tune1));
    if (const char *env = sw_env("STX_AUTOTUNE")) e->autotune = atoi(env) != 0;
    if (const char *env = sw_env("STX_POOL_CODES")) e->pool_codes = atoi(env) != 0;
    if (const char *env = sw_env("STX_WINOGRAD")) e->winograd = atoi(env) != 0;
    e->scalars_cap = kScalarFloats;
    for (stx_engine::ScalarArena &a : e->arena) {
        STX_TRY(a.scalars.ensure(e->scalars_cap * sizeof(float)));
        STX_HIP(hipHostMalloc(reinterpret_cast<void **>(&a.host), e->scalars_cap * sizeof(float),
                              hipHostMallocDefault));
        STX_TRY(a.dscalars.ensure(e->dscalars_cap * sizeof(double)));
        STX_HIP(hipHostMalloc(reinterpret_cast<void **>(&a.dhost), e->dscalars_cap * sizeof(double),
                              hipHostMallocDefault));
        STX_HIP(hipEventCreateWithFlags(&a.fence, hipEventDisableTiming));
    }
    STX_TRY(e->red_scratch.ensure(9 * kBlocks * sizeof(float)));   // nine sums: stx_image_color_stats
    {
        std::lock_guard<std::mutex> lock(e->sh->mutex);
        e->sh->members.push_back(e.get());
    }
    *out = e.release();
    return STX_OK;
}

extern "C" {

int stx_engine_create(int device, const stx_layer_desc *layers, int n_layers, stx_engine **out) {
    return build_engine(device, layers, n_layers, nullptr, out);
}

int stx_engine_create_shared(stx_engine *primary, stx_engine **out) {
    if (!primary || !out) {
        set_error("stx_engine_create_shared: bad arguments");
        return STX_ERR_ARG;
    }
    std::vector<stx_layer_desc> descs(primary->layers.size());
    for (size_t i = 0; i < descs.size(); ++i) {
        const Layer &L = primary->layers[i];
        stx_layer_desc &d = descs[i];
        d.name = L.name.c_str();
        d.type = L.type;
        d.bottom = L.bottom.empty() ? nullptr : L.bottom.c_str();
        d.top = L.top.c_str();
        d.num_output = i == 0 ? primary->blobs[L.top_blob].channels : L.num_output;
        d.kernel_size = L.ksize;
        d.pad = L.pad;
        d.stride = L.stride;
        d.pool_mode = L.pool_mode;
    }
    // every filter bank the group has packed so far (and its weights and targets) is complete
    // before the new member's stream can touch it
    STX_TRY(primary->set_device());
    for (stx_engine *m : primary->sh->members) STX_HIP(hipStreamSynchronize(m->stream));
    return build_engine(primary->device, descs.data(), (int)descs.size(), primary->sh, out);
}

void stx_engine_destroy(stx_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto &b : e->sgrad) b->release();
    e->marks_buf.release();
    e->amax.release();
    e->audit_buf.release();
    for (Blob &b : e->blobs) {
        b.data.release();
        b.diff.release();
        b.codes.release();
        b.relu_codes.release();
    }
    for (hipEvent_t ev : e->fence_events) (void)hipEventDestroy(ev);
    bool last;
    {
        std::lock_guard<std::mutex> lock(e->sh->mutex);
        auto &m = e->sh->members;
        m.erase(std::remove(m.begin(), m.end(), e), m.end());
        last = m.empty();
    }
    if (last) {     // the shared state goes with its last engine
        for (auto &kv : e->sh->conv) {
            kv.second.w.release();
            kv.second.b.release();
            for (auto &p : kv.second.packed) p.second->release();
        }
        clear_all_targets(*e->sh);
    }
    DevBuf *bufs[] = {&e->cx_io, &e->shift_io, &e->selfsim_io, &e->swd_work, &e->swd_io, &e->nnfm_scratch, &e->stat_scratch, &e->masked_feat, &e->masked_target, &e->splitk, &e->gram_partials, &e->gram, &e->dsym, &e->dsym_pieces, &e->symm_partials,
                      &e->upload, &e->red_scratch, &e->swt_scratch, &e->lap_scratch, &e->flow_work, &e->poisson_work, &e->first_gram, &e->color_sums};
    for (DevBuf *b : bufs) b->release();
    for (stx_engine::SwtTable &t : e->swt_tables) t.taps.release();
    for (stx_engine::ScalarArena &a : e->arena) {
        a.scalars.release();
        a.dscalars.release();
        if (a.host) (void)hipHostFree(a.host);
        if (a.dhost) (void)hipHostFree(a.dhost);
        if (a.fence) (void)hipEventDestroy(a.fence);
    }
    for (auto &pe : e->prof) {
        (void)hipEventDestroy(pe.start);
        (void)hipEventDestroy(pe.stop);
    }
    for (hipEvent_t ev : e->event_pool) (void)hipEventDestroy(ev);
    for (int i = 0; i < stx_engine::kTimed; ++i) {
        if (e->ev_start[i]) (void)hipEventDestroy(e->ev_start[i]);
        if (e->ev_stop[i]) (void)hipEventDestroy(e->ev_stop[i]);
    }
    if (e->ev_tune0) (void)hipEventDestroy(e->ev_tune0);
    if (e->ev_tune1) (void)hipEventDestroy(e->ev_tune1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int stx_set_conv_weights(stx_engine *e, const char *conv_layer, const float *weights,
                         const float *bias, int mem) {
    if (!e || !conv_layer || !weights) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    auto it = e->layer_index.find(conv_layer);
    if (it == e->layer_index.end() || e->layers[it->second].type != STX_LAYER_CONV) {
        set_error("stx_set_conv_weights: '%s' is not a convolution layer", conv_layer);
        return STX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lock(e->sh->mutex);
    const bool shared = e->sh->members.size() > 1;
    if (shared) STX_TRY(quiesce_members(e));
    ConvParams &cp = e->sh->conv[it->second];
    const size_t nw = (size_t)cp.cout * cp.cin * cp.ks * cp.ks;
    STX_TRY(cp.w.ensure(nw * sizeof(float)));
    STX_TRY(cp.b.ensure((size_t)cp.cout * sizeof(float)));
    STX_TRY(copy_in(e, cp.w.ptr, weights, mem, nw * sizeof(float)));
    if (bias)
        STX_TRY(copy_in(e, cp.b.ptr, bias, mem, (size_t)cp.cout * sizeof(float)));
    else
        STX_HIP(hipMemsetAsync(cp.b.ptr, 0, (size_t)cp.cout * sizeof(float), e->stream));
    // host buffers may be reused by the caller right away; engines sharing the bank read it from
    // their own streams
    if (mem == STX_HOST || shared) STX_HIP(hipStreamSynchronize(e->stream));
    for (auto &p : cp.packed) p.second->release();
    cp.packed.clear();
    cp.set = true;
    return STX_OK;
}

int stx_sync(stx_engine *e) {
    if (!e) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return do_sync(e);
}

int stx_fence(stx_engine *e, unsigned long long *ticket) {
    if (!e || !ticket) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    stx_engine::ScalarArena &a = e->A();
    STX_HIP(hipEventRecord(a.fence, e->stream));
    a.ticket = e->next_ticket++;
    *ticket = a.ticket;
    e->cur ^= 1;
    stx_engine::ScalarArena &b = e->A();
    if (b.ticket) {      // nobody waited for the arena that is about to be reused: publish it now
        STX_HIP(hipEventSynchronize(b.fence));
        publish_arena(b);
    }
    return STX_OK;
}

int stx_fence_wait(stx_engine *e, unsigned long long ticket) {
    if (!e) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    for (stx_engine::ScalarArena &a : e->arena) {
        if (a.ticket && a.ticket == ticket) {
            STX_HIP(hipEventSynchronize(a.fence));
            publish_arena(a);
        }
    }
    return STX_OK;      // (an older ticket: published long ago)
}

int stx_engine_device(stx_engine *e, int *device) {
    if (!e || !device) return STX_ERR_ARG;
    *device = e->device;
    return STX_OK;
}

int stx_engine_stream(stx_engine *e, void **hip_stream) {
    if (!e || !hip_stream) return STX_ERR_ARG;
    *hip_stream = e->stream;
    return STX_OK;
}

int stx_engine_wait(stx_engine *e, stx_engine *other) {
    if (!e || !other) return STX_ERR_ARG;
    if (e == other) return STX_OK;
    constexpr size_t kRing = 16;    // a wait reads the event's state when it is queued: re-recording later is safe
    STX_TRY(other->set_device());
    if (other->fence_events.size() < kRing) {
        hipEvent_t ev;
        STX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        other->fence_events.push_back(ev);
        other->fence_next = other->fence_events.size() - 1;
    }
    hipEvent_t ev = other->fence_events[other->fence_next];
    other->fence_next = (other->fence_next + 1) % kRing;
    STX_HIP(hipEventRecord(ev, other->stream));
    STX_TRY(e->set_device());
    STX_HIP(hipStreamWaitEvent(e->stream, ev, 0));
    return STX_OK;
}

int stx_engine_query(stx_engine *e, int what, double *value) {
    if (!e || !value) return STX_ERR_ARG;
    std::lock_guard<std::mutex> lock(e->sh->mutex);
    switch (what) {
        case STX_Q_SHARED_ENGINES: *value = (double)e->sh->members.size(); break;
        case STX_Q_TARGET_UPLOADS: *value = (double)e->sh->target_uploads; break;
        case STX_Q_TARGET_BYTES: *value = e->sh->target_bytes; break;
        case STX_Q_WEIGHT_BYTES: {
            double b = 0;
            for (auto &kv : e->sh->conv) {
                b += (double)kv.second.w.bytes + (double)kv.second.b.bytes;
                for (auto &p : kv.second.packed) b += (double)p.second->bytes;
            }
            *value = b;
            break;
        }
        case STX_Q_TILE_EVALS: *value = (double)e->n_tile_evals; break;
        case STX_Q_PEERS_WITHOUT_ACCESS: *value = (double)peers_without_access(e->device); break;
        case STX_Q_TILE_IO_DIRECT: *value = (double)e->n_tile_io_direct; break;
        case STX_Q_INJECT_SPECIALISED: *value = (double)e->n_inject_specialised; break;
        case STX_Q_INJECT_VARIANTS: *value = (double)e->inject_variants; break;
        default:
            set_error("stx_engine_query: unknown item %d", what);
            return STX_ERR_ARG;
    }
    return STX_OK;
}

int stx_malloc(stx_engine *e, size_t bytes, void **dev_ptr) {
    if (!e || !dev_ptr) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    hipError_t err = hipMalloc(dev_ptr, bytes ? bytes : 4);
    if (err != hipSuccess) {
        set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(err));
        return STX_ERR_NOMEM;
    }
    return STX_OK;
}

int stx_free(stx_engine *e, void *dev_ptr) {
    if (!e) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    if (dev_ptr) STX_HIP(hipFree(dev_ptr));
    return STX_OK;
}

int stx_memset_async(stx_engine *e, void *dev_ptr, int value, size_t bytes) {
    if (!e || !dev_ptr) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_HIP(hipMemsetAsync(dev_ptr, value, bytes, e->stream));
    return STX_OK;
}

int stx_memcpy_async(stx_engine *e, void *dst, int dst_mem, const void *src, int src_mem,
                     size_t bytes) {
    if (!e || !dst || !src) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    hipMemcpyKind kind = hipMemcpyDefault;
    if (dst_mem == STX_HOST && src_mem == STX_HOST) kind = hipMemcpyHostToHost;
    if (dst_mem == STX_HOST && src_mem == STX_DEVICE) kind = hipMemcpyDeviceToHost;
    if (dst_mem == STX_DEVICE && src_mem == STX_HOST) kind = hipMemcpyHostToDevice;
    STX_HIP(hipMemcpyAsync(dst, src, bytes, kind, e->stream));
    return STX_OK;
}

int stx_profile_enable(stx_engine *e, int on) {
    if (!e) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_HIP(hipStreamSynchronize(e->stream));
    for (auto &pe : e->prof) {
        e->event_pool.push_back(pe.start);
        e->event_pool.push_back(pe.stop);
    }
    e->prof.clear();
    e->profiling = on != 0;
    return STX_OK;
}

int stx_profile_read(stx_engine *e, char *buf, size_t buf_len, size_t *needed) {
    if (!e || (!buf && buf_len)) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_HIP(hipStreamSynchronize(e->stream));
    std::string out;
    std::vector<long long> marks((size_t)e->marks_used * 2);
    if (!marks.empty())
        STX_HIP(hipMemcpy(marks.data(), e->marks_buf.ptr, marks.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (auto &pe : e->prof) {
        float ms = 0.f;
        STX_HIP(hipEventElapsedTime(&ms, pe.start, pe.stop));
        double mhz = 0.0;      // the shader clock inside the group's convolution kernel (stx_clock_marks)
        if (pe.mark >= 0 && (size_t)pe.mark * 2 + 1 < marks.size() && marks[2 * pe.mark + 1] > 0)
            mhz = (double)marks[2 * pe.mark] / (double)marks[2 * pe.mark + 1] * 100.0;
        char line[256];
        snprintf(line, sizeof line, "%s\t%.6f\t%.6e\t%.1f\n", pe.label.c_str(), ms, pe.flops, mhz);
        out += line;
        e->event_pool.push_back(pe.start);
        e->event_pool.push_back(pe.stop);
    }
    e->prof.clear();
    if (needed) *needed = out.size() + 1;
    if (buf_len) {
        const size_t n = std::min(buf_len - 1, out.size());
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return STX_OK;
}

int stx_amax_audit(stx_engine *e, int on) {
    if (!e) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_HIP(hipStreamSynchronize(e->stream));
    e->audit.clear();
    e->amax_audit = false;
    if (on)
        STX_TRY(e->audit_buf.ensure(kMaxAmaxAudit * 2 * kAmaxSlots * sizeof(unsigned)));
    else
        e->audit_buf.release();
    e->amax_audit = on != 0;
    return STX_OK;
}

int stx_amax_audit_read(stx_engine *e, char *buf, size_t buf_len, size_t *needed) {
    if (!e || (!buf && buf_len)) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_HIP(hipStreamSynchronize(e->stream));
    std::string out;
    std::vector<unsigned> words(e->audit.size() * 2 * kAmaxSlots);
    if (!words.empty())
        STX_HIP(hipMemcpy(words.data(), e->audit_buf.ptr, words.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < e->audit.size(); ++i) {
        const stx_engine::AuditEntry &a = e->audit[i];
        const unsigned *rec = words.data() + 2 * i * kAmaxSlots, *meas = rec + kAmaxSlots;
        const unsigned recorded = *std::max_element(rec, rec + kAmaxSlots);
        const unsigned measured = *std::max_element(meas, meas + kAmaxSlots);
        char line[256];
        snprintf(line, sizeof line, "%s\t%s\t%s\t%s\t%08x\t%08x\n", a.consumer.c_str(), a.blob.c_str(),
                 a.diff ? "diff" : "data", a.source.c_str(), recorded, measured);
        out += line;
    }
    e->audit.clear();
    if (needed) *needed = out.size() + 1;
    if (buf_len) {
        const size_t n = std::min(buf_len - 1, out.size());
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return STX_OK;
}

int stx_last_tile_ms(stx_engine *e, float *ms) {
    if (!e || !ms) return STX_ERR_ARG;
    if (!e->timed) {
        set_error("stx_last_tile_ms: no tile has been evaluated");
        return STX_ERR_STATE;
    }
    STX_TRY(e->set_device());
    // the newest call that has finished; if none of the last few has, wait for the newest
    // (only slots that were recorded: hipEventQuery calls a never-recorded event complete, and
    // hipEventElapsedTime then fails on it)
    int pick = e->ev_cur;
    for (int k = 0; k < e->ev_recorded; ++k) {
        const int i = (e->ev_cur - k + stx_engine::kTimed) % stx_engine::kTimed;
        const hipError_t q = hipEventQuery(e->ev_stop[i]);
        if (q == hipSuccess) {
            pick = i;
            break;
        }
        (void)hipGetLastError();      // hipErrorNotReady
    }
    STX_HIP(hipEventSynchronize(e->ev_stop[pick]));
    STX_HIP(hipEventElapsedTime(ms, e->ev_start[pick], e->ev_stop[pick]));
    return STX_OK;
}

int stx_clock_marks(stx_engine *e, int on) {
    if (!e) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    if (on) {
        STX_TRY(e->marks_buf.ensure((size_t)kMaxClockMarks * 2 * sizeof(long long)));
        STX_HIP(hipMemsetAsync(e->marks_buf.ptr, 0, (size_t)kMaxClockMarks * 2 * sizeof(long long), e->stream));
    }
    e->clock_marks = on != 0;
    return STX_OK;
}

int stx_clock_marks_read(stx_engine *e, double *mhz, int max_values, int *n_values) {
    if (!e || !mhz || !n_values || max_values < 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_HIP(hipStreamSynchronize(e->stream));
    const int n = std::min(max_values, e->marks_used);
    std::vector<long long> h((size_t)n * 2);
    if (n) STX_HIP(hipMemcpy(h.data(), e->marks_buf.ptr, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) mhz[i] = h[2 * i + 1] > 0 ? (double)h[2 * i] / (double)h[2 * i + 1] * 100.0 : 0.0;
    *n_values = n;
    e->marks_used = 0;
    return STX_OK;
}

int stx_last_tile_flops(stx_engine *e, double *algorithmic, double *issued) {
    if (!e || !algorithmic || !issued) return STX_ERR_ARG;
    if (!e->timed) {
        set_error("stx_last_tile_flops: no tile has been evaluated");
        return STX_ERR_STATE;
    }
    *algorithmic = e->flop_algorithmic;
    *issued = e->flop_issued;
    return STX_OK;
}

}  // extern "C"
