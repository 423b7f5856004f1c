/*
 * stx.h -- C ABI of libstx, the MI355X (gfx950) tile engine for tiled neural style transfer.
 *
 * This is the drop-in boundary for the hot path of crowsonkb/style_transfer.  The reference has
 * no native plugin ABI; its hot path sits behind the tile-worker message protocol
 * (style_transfer.py:156-166), served by TileWorker.process_one_request (style_transfer.py:215-259)
 * which calls CaffeModel.eval_features_tile / eval_sc_grad_tile (style_transfer.py:421-427,
 * 556-612), and behind the host-side numpy in eval_loss_and_grad (style_transfer.py:700-736) and
 * optimizers.py.  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - every function returns STX_OK (0) or a negative stx_status; nothing throws or aborts across
 *     the ABI; stx_last_error() gives the message of the calling thread's last failure;
 *   - plain pointers and sizes only.  A pointer argument that may live on either side carries an
 *     stx_mem tag: STX_HOST (pageable or pinned host memory) or STX_DEVICE (memory of the engine's
 *     GPU, e.g. from stx_malloc or any HIP allocation of this process);
 *   - buffers are caller-owned; float tensors are dense row-major float32 in the reference's
 *     layouts: images [3][H][W] (BGR, mean-subtracted), feature maps [C][h][w], Grams [C][C];
 *   - an engine owns one GPU and one HIP stream.  Calls on one engine are issued in order on that
 *     stream and are ASYNCHRONOUS w.r.t. the host unless stated; stx_sync() waits and then
 *     publishes pending scalar results (losses).  Engines on different GPUs are independent --
 *     that independence is the whole multi-GPU story (tiles never exchange data);
 *   - one host thread per engine at a time.
 */
#ifndef STX_H_
#define STX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct stx_engine stx_engine;

typedef enum stx_status {
    STX_OK = 0,
    STX_ERR_ARG = -1,          /* bad argument (null pointer, unknown layer name, bad shape) */
    STX_ERR_HIP = -2,          /* a HIP runtime call or kernel launch failed */
    STX_ERR_STATE = -3,        /* call sequence error (e.g. weights or targets not set) */
    STX_ERR_UNSUPPORTED = -4,  /* graph / parameter outside what the kernels implement */
    STX_ERR_NOMEM = -5
} stx_status;

typedef enum stx_mem { STX_HOST = 0, STX_DEVICE = 1 } stx_mem;

typedef enum stx_layer_type {
    STX_LAYER_INPUT = 0, STX_LAYER_CONV = 1, STX_LAYER_RELU = 2, STX_LAYER_POOL = 3
} stx_layer_type;

typedef enum stx_pool_mode { STX_POOL_MAX = 0, STX_POOL_AVE = 1 } stx_pool_mode;

/* One layer of a Caffe deploy.prototxt (vgg19.prototxt:3-342): same names, same graph. */
typedef struct stx_layer_desc {
    const char *name;       /* layer name, e.g. "conv1_1", "relu1_1", "pool1" */
    int type;               /* stx_layer_type */
    const char *bottom;     /* input blob name (NULL for the input layer) */
    const char *top;        /* output blob name; ReLU must be in-place (top == bottom) */
    int num_output;         /* conv: output channels; input layer: image channels (3) */
    int kernel_size;        /* conv: 3 (pad 1) or 1 (pad 0); pool: 2 */
    int pad;                /* conv */
    int stride;             /* pool: 2 */
    int pool_mode;          /* stx_pool_mode */
} stx_layer_desc;

/* ---------------------------------------------------------------- library / device queries */
const char *stx_version(void);
/* Message of the calling thread's most recent failing call ("" if none). */
const char *stx_last_error(void);
/* The library's STX_* switches (A/B levers, test hooks) are read from a snapshot of
 * the environment taken at first use, not with getenv() at every launch; a program that changes one while it
 * runs calls this to take a new snapshot.  (No counterpart in the reference: its only run-time switches are the
 * command line's, config_system.py:26-118.) */
int stx_reread_env(void);
/* Number of visible GPUs; replaces detect_devices() (config_system.py:17-24, nvidia-smi -L). */
int stx_device_count(int *count);
/* gcnArchName of a device (e.g. "gfx950:sramecc+:xnack-") into buf. */
int stx_device_name(int device, char *buf, size_t buf_len);

/* ------------------------------------------------------------------------ engine lifetime */
/* Replaces TileWorker.run's setup (style_transfer.py:187-207: pick device, caffe.Net(deploy, 1,
 * weights)).  The graph is copied.  Weights are supplied separately with stx_set_conv_weights. */
int stx_engine_create(int device, const stx_layer_desc *layers, int n_layers, stx_engine **out);
/* Another worker on the primary's GPU: its own HIP stream and activation buffers, but the
 * primary's network, weights, packed filter banks and targets (one copy per GPU).  The reference
 * gives every TileWorker process its own caffe.Net (style_transfer.py:187-207) and sends the
 * targets to each (style_transfer.py:309-332); engines created here see what is set through any
 * engine of the group -- stx_set_conv_weights / stx_set_contents_and_styles need to be called
 * once per GPU. */
int stx_engine_create_shared(stx_engine *primary, stx_engine **out);
void stx_engine_destroy(stx_engine *e);
/* Caffe blob layout: weights [Cout][Cin][k][k], bias [Cout], float32 (Appendix C of SURVEY.md). */
int stx_set_conv_weights(stx_engine *e, const char *conv_layer, const float *weights,
                         const float *bias, int mem);
/* Waits for all work queued on the engine, then writes pending loss values. */
int stx_sync(stx_engine *e);
/* A step loop that runs AHEAD of the GPU.  The reference's loop blocks on every iteration's loss
 * and statistics before it starts the next one (style_transfer.py:799-815: resp_q.get(), then the
 * callback); here the host may queue iteration i + 1 first and collect iteration i afterwards.
 * stx_fence closes the engine's current set of pending loss values behind an event on its stream
 * and returns a ticket; calls queued after it collect theirs in a second set.  stx_fence_wait
 * waits for that event only -- not for the work queued since -- and writes the values of the set
 * the ticket names (a ticket that was already published, by stx_sync or because its set had to
 * be reused, is a no-op).  At most one closed set exists per engine: a second stx_fence before
 * the first was waited for publishes the older set itself (after waiting for it). */
int stx_fence(stx_engine *e, unsigned long long *ticket);
int stx_fence_wait(stx_engine *e, unsigned long long ticket);
/* Orders e's stream behind everything queued so far on other's stream (an event; no host wait).
 * The engines may sit on different GPUs.  This is what replaces the reference's blocking
 * resp_q.get() between handing out tiles and stitching their gradients (style_transfer.py:
 * 634-643): the master's stream waits for a worker's gradient, the host does not. */
int stx_engine_wait(stx_engine *e, stx_engine *other);
/* Counters for tests and bench.py. */
typedef enum stx_query {
    STX_Q_SHARED_ENGINES = 0,  /* engines sharing this engine's weights / targets (>= 1) */
    STX_Q_TARGET_UPLOADS = 1,  /* stx_set_contents_and_styles calls served by this group */
    STX_Q_TARGET_BYTES = 2,    /* bytes those calls copied, cumulative */
    STX_Q_WEIGHT_BYTES = 3,    /* device bytes of weights + packed banks held by this group */
    STX_Q_TILE_EVALS = 4,      /* stx_sc_grad_tile calls enqueued by this engine */
    STX_Q_PEERS_WITHOUT_ACCESS = 5, /* GPUs of the node this engine's GPU has no direct (xGMI peer)
                                     * access to: copies to / from them are staged by the runtime
                                     * (reported once on stderr) */
    STX_Q_TILE_IO_DIRECT = 6,  /* ends of this engine's stx_sc_grad_tile calls (the tile in, the gradient out:
                                * up to two per call) that worked on the caller's buffers without a copy */
    STX_Q_INJECT_SPECIALISED = 7,   /* backward convolutions this engine launched with a specialised body of
                                     * the loss-injecting epilogue */
    STX_Q_INJECT_VARIANTS = 8  /* ... and which: bit v is set once body v has run (v = 1 style term | 2 content
                                * term, + 4 masked by ReLU nibbles | 8 by the fp32 blob) */
} stx_query;
int stx_engine_query(stx_engine *e, int what, double *value);
int stx_engine_device(stx_engine *e, int *device);
/* The engine's hipStream_t as an opaque pointer (for callers that enqueue their own copies). */
int stx_engine_stream(stx_engine *e, void **hip_stream);

/* ---------------------------------------------------------------------------- raw memory */
int stx_malloc(stx_engine *e, size_t bytes, void **dev_ptr);
int stx_free(stx_engine *e, void *dev_ptr);
int stx_memset_async(stx_engine *e, void *dev_ptr, int value, size_t bytes);
/* dst/src tagged with stx_mem; device<->device copies may cross GPUs (xGMI peer copy). */
int stx_memcpy_async(stx_engine *e, void *dst, int dst_mem, const void *src, int src_mem,
                     size_t bytes);

/* ------------------------------------------------------------------- targets (per scale) */
/* One content feature map: ContentData.features[layer] (style_transfer.py:165,246-249), the
 * FULL-image map [C][h][w] with h = ceil(H/scale), w = ceil(W/scale) (style_transfer.py:440). */
typedef struct stx_content_target {
    int content_index;      /* index into model.contents (normally 0) */
    const char *layer;
    int channels, height, width;
    const float *features;
    int mem;
} stx_content_target;

/* One style Gram: StyleData.grams[layer] (style_transfer.py:166,250-253), [C][C], only the lower
 * triangle is read (num_utils.py:53-66). */
typedef struct stx_style_target {
    int style_index;        /* index into model.styles (normally 0) */
    const char *layer;
    int channels;
    const float *gram;
    int mem;
} stx_style_target;

/* Replaces the SetContentsAndStyles message (style_transfer.py:163,243-254,309-332): replaces all
 * targets held by the engine.  Data is copied before the call returns control of the buffers
 * (host sources: synchronously; device sources: ordered on the engine stream). */
int stx_set_contents_and_styles(stx_engine *e, const stx_content_target *contents, int n_contents,
                                const stx_style_target *styles, int n_styles);

/* Spatial control (Gatys et al., "Controlling Perceptual Factors in Neural Style Transfer"; no
 * counterpart in the reference, whose styles act on the whole picture): style `style_index` applies
 * where its mask is white.  mask is [H][W] float32 in [0, 1] (values are not checked), H x W the image
 * frame of the current targets.  For a style layer b of scale s the library keeps the mask map
 *   m_b[y][x] = mean of mask over [y s, min((y + 1) s, H)) x [x s, min((x + 1) s, W)),
 * ceil(H/s) x ceil(W/s) (receptive-field growth is ignored), and a tile evaluation takes the tile's window
 * of it exactly as a content map's (start // s, roll // s, wrapping; the same range error).  With F the
 * tile's blob [C][fh][fw], HW = fh fw, m that window and Gs the style's Gram (of the WHOLE style picture):
 *   a     = sum m^2 / HW
 *   Fm    = F . m                                     (every channel)
 *   D     = tril(Fm Fm^T)/(C HW) - a Gs
 *   loss += lw sw[b] 1/2 |D|^2 / n_styles
 *   S     = m . (sym(D) Fm)
 *   diff += lw sw[b] / n_styles * a S / (sum|S| / S.size + EPS)
 * m == 1 is the unmasked term bit for bit; m == 0 adds nothing (0 / EPS).  The factor a keeps the
 * per-pixel strength inside a region what it is in an unmasked run.  Styles without a mask are untouched. */
typedef struct stx_style_mask {
    int style_index;        /* the style_index of the stx_style_target entries it restricts */
    int H, W;
    const float *mask;
    int mem;
} stx_style_mask;
/* Replaces all masks of the engine's group (n = 0: none).  Call it after stx_set_contents_and_styles,
 * which clears them: the maps are built for every layer that has a style target of that index and are
 * shared like the targets (stx_engine_create_shared).  A mask of another size than the content frame
 * surfaces as the window range error at evaluation. */
int stx_set_style_masks(stx_engine *e, const stx_style_mask *masks, int n);

/* Spatial control of the content term (not in the reference; Gatys et al., "Controlling Perceptual Factors in
 * Neural Style Transfer"): a greyscale mask in the content picture's frame, values in [0, 1], says where the
 * content picture is held (white) and where the content term is off (black).  For a blob of scale s that has a
 * content target the library keeps the block means of the mask, ceil(H/s) x ceil(W/s) -- the size of the
 * blob's content maps -- and a tile evaluation takes the tile's window of it with the very window of the content
 * map (start // s, roll // s, wrapping; the same range error).  With F the tile's blob [C][fh][fw], c the
 * window of the content map and m that of the mask map (every channel):
 *   d     = F - c
 *   a     = sum m / (fh fw)                           (the window's mean weight)
 *   loss += lw cw[b] 1/2 sum m d^2
 *   S0    = m d
 *   diff += lw cw[b] * a S0 / (sum|S0| / S0.size + EPS)
 * m == 1 is the unmasked term (its sums bit for bit); m == 0 adds nothing (0 / EPS); a uniform m == k is the
 * unmasked term with the content weight scaled by k, up to the EPS term -- the normalisation would otherwise
 * undo the mask's overall level, which is what a is for.  One mask applies to every content target.
 *
 * mask == NULL clears.  Call it after stx_set_contents_and_styles, which clears the maps: they are built for
 * every blob that has a content target and are shared like the targets (stx_engine_create_shared).  A mask
 * whose map at such a blob has another size than the blob's content maps is STX_ERR_ARG here. */
int stx_set_content_mask(stx_engine *e, const float *mask, int H, int W, int mem);

/* The mean / std style term (not in the reference): the BN-statistics loss of Li et al., "Demystifying
 * Neural Style Transfer", the quantity AdaIN aligns.  A tapped blob F [C][h][w] -- the array the Gram term
 * reads -- is held to per-channel targets MU, SD.  With n = h w and eps = 1e-5:
 *   mu_c  = (1/n) sum_x F_c(x)
 *   var_c = (1/n) sum_x (F_c(x) - mu_c)^2                  (population variance)
 *   sd_c  = sqrt(var_c + eps)
 *   E     = sum_c [ (mu_c - MU_c)^2 + (sd_c - SD_c)^2 ]
 *   S_c(x) = (mu_c - MU_c) + (sd_c - SD_c) (F_c(x) - mu_c) / sd_c        ( = n d(E/2)/dF_c(x) )
 *   loss        += lw weight E / 2
 *   diff[layer] += lw weight S / (sum|S| / (C n) + EPS)
 * The last line is the reference's normalize, exactly as for the Gram term (EPS: float32 epsilon).  A
 * tile's statistics are the tile's own, as its Gram is.  mu and sd are rounded to float32 once and
 * everything else is formed from the rounded values: a tile whose statistics equal the targets (those
 * stx_feature_stats gives for the same array) contributes exactly 0 to the loss and to the gradient.
 * No atomics; the partial sums are added in a fixed order: the same inputs give the same bits. */
typedef struct stx_stat_target {
    const char *layer;
    int channels;
    const float *mean;      /* [channels] */
    const float *sd;        /* [channels] */
    int mem;
    double weight;
} stx_stat_target;
/* Replaces all statistics targets of the engine's group (n = 0: none); one per layer at most.  They are
 * shared like the style targets (stx_engine_create_shared) and stx_set_contents_and_styles clears them:
 * call this behind it.  A channel count other than the layer's is STX_ERR_ARG here.  A layer with a
 * target is part of every stx_sc_grad_tile evaluation: with the layer_weight of its tap if the tap list
 * names it (whatever else the tap asks for, nothing included), with lw = 1 otherwise; a tap list without
 * a content, style or Deep-Dream layer is then accepted, an empty one (n_taps = 0) too; the tapped layers
 * and these still lie on one path (STX_ERR_UNSUPPORTED otherwise, at the evaluation).  The term follows the blob's style terms in the loss and in the gradient, in the same order on
 * every call. */
int stx_set_stat_targets(stx_engine *e, const stx_stat_target *targets, int n);

/* The nearest-neighbour feature matching term (NNFM; not in the reference): the per-pixel style loss of ARF,
 * NNST and STROTSS-style tools.  Every column f_i of a tapped blob F [C][h][w] -- the array the Gram term
 * reads, n = h w columns -- is pulled towards the most similar row of a fixed bank B [rows][C] whose rows b_j
 * have unit length or are all zero:
 *   r_i  = |f_i|,  x_i = f_i / r_i           (a column with r_i = 0: x_i = 0, c_i = 0, j_i = 0, S_i = 0)
 *   j_i  = argmax_j x_i . b_j                (the LOWEST j among equal scores)
 *   c_i  = x_i . b_{j_i}
 *   E    = (2/n) sum_i (1 - c_i)             ( = mean |x_i - b_{j_i}|^2 for unit rows; E / 2 is ARF's loss )
 *   S_i  = -(b_{j_i} - c_i x_i) / r_i        ( = n d(E/2)/d f_i with j_i held fixed )
 *   loss        += lw weight E / 2
 *   diff[layer] += lw weight S / (sum|S| / (C n) + EPS)
 * The last line is the reference's normalize, exactly as for the Gram term.  The search runs on the fp16
 * matrix pipe with two-piece operands (three products, fp32 accumulation): j_i is the float64 argmax up to
 * scores closer than about 1e-6.  c_i, E and S are recomputed in float32 from (F, B, j_i) alone.  The term is
 * per pixel: a tile's term is the tile's own and tiles exchange nothing.  No atomics; the same inputs give
 * the same bits.  channels must be a multiple of 64 and rows x channels, n x channels stay below 2^31
 * (STX_ERR_UNSUPPORTED otherwise). */
typedef struct stx_nnfm_target {
    const char *layer;
    int channels;
    int rows;
    const float *bank;      /* [rows][channels] */
    int mem;
    double weight;
} stx_nnfm_target;
/* Replaces all NNFM banks of the engine's group (n = 0: none); one per layer at most.  The bank is copied and
 * its fp16 pieces are built once, here; the source may be freed when the call returns.  The banks are shared
 * like the style targets (stx_engine_create_shared) and stx_set_contents_and_styles clears them: call this
 * behind it.  A layer with a bank is part of every stx_sc_grad_tile evaluation under the rules of
 * stx_set_stat_targets: the layer_weight of its tap if the tap list names it, lw = 1 otherwise, and all
 * layers on one path.  The term follows the blob's statistics term in the loss and in the gradient. */
int stx_set_nnfm_targets(stx_engine *e, const stx_nnfm_target *targets, int n);

/* The same term over 3 x 3 patches (CNNMRF, NNST): pixel p = (y, x) of the blob has the patch
 *   P_p[t, c] = F[c][y + dy][x + dx]         t = (dy, dx), dy and dx in {-1, 0, 1}; 0 outside the map
 * a 9 C vector in tap-major order: dy outer, dx inner, (-1, -1) first, then the channel.  Every pixel has a
 * patch (n of them) and a bank row is a unit or all-zero 9 C vector in the same order:
 *   R_p  = |P_p|,  X_p = P_p / R_p           (R_p = 0: c_p = 0, j_p = 0, no gradient from this patch)
 *   j_p  = argmax_j P_p . b_j                (the LOWEST j among equal scores)
 *   c_p  = X_p . b_{j_p}
 *   E    = (2/n) sum_p (1 - c_p)
 *   G_p  = -(b_{j_p} - c_p X_p) / R_p        (9 C: n d(E/2)/dP_p with j_p held fixed)
 *   S[c][p] = sum_t G_{p - t}[t, c]          over the taps whose centre p - t lies in the map
 * and loss, diff as above.  A tile's border patches are padded with zeros: tiles stay independent.
 * patch: 1 (the term above, byte for byte what stx_set_nnfm_targets does) or 3; anything else is STX_ERR_ARG.
 * channels must be a multiple of 64, and rows x patch^2 x channels, n x channels stay below 2^31
 * (STX_ERR_UNSUPPORTED otherwise). */
typedef struct stx_nnfm_patch_target {
    const char *layer;
    int channels;
    int patch;
    int rows;
    const float *bank;      /* [rows][patch * patch * channels] */
    int mem;
    double weight;
} stx_nnfm_patch_target;
/* stx_set_nnfm_targets for banks of either kind: a layer has ONE bank, patch or plain, and either call
 * replaces the whole set. */
int stx_set_nnfm_patch_targets(stx_engine *e, const stx_nnfm_patch_target *targets, int n);

/* The same term against the k best rows instead of one (patch-based synthesis, NNST): with K = min(k, rows),
 *   J_i  = (j_i1 ... j_iK)                   the K rows with the best scores x_i . b_j, ordered by score
 *                                            descending, and among equal scores the LOWER index first
 *   t_i  = (1/K) sum_r b_{j_ir}              (float32, added in rank order, then scaled)
 *   c_i  = x_i . t_i,   E = (2/n) sum_i (1 - c_i)      ( = the mean over i and r of |x_i - b_{j_ir}|^2 )
 *   S_i  = -(t_i - c_i x_i) / r_i            (n d(E/2)/df_i with J_i held fixed)
 * and loss, diff as above; with patch 3, x_i and r_i are X_p and R_p and G_p is folded into S as above.  A zero
 * column takes the rows 0 .. K - 1, c = 0, S = 0.  The search's matrix work is done once whatever k is.
 * k: 1 (stx_set_nnfm_patch_targets, byte for byte) to 4; anything else is STX_ERR_ARG.  Every other refusal is
 * that of stx_set_nnfm_patch_targets. */
typedef struct stx_nnfm_knn_target {
    const char *layer;
    int channels;
    int patch;
    int k;
    int rows;
    const float *bank;      /* [rows][patch * patch * channels] */
    int mem;
    double weight;
} stx_nnfm_knn_target;
/* stx_set_nnfm_targets for banks of any kind: a layer has ONE bank, and any of the three calls replaces the
 * whole set. */
int stx_set_nnfm_knn_targets(stx_engine *e, const stx_nnfm_knn_target *targets, int n);

/* The same term with a coverage part (the other half of STROTSS's relaxed earth mover's distance): every bank row
 * also looks for ITS most similar column and pulls that one towards itself, so that rows no column picked still
 * act on the result.  With lambda = cover and E_fwd, S_fwd the term above (any k):
 *   i*_j    = argmax_i x_i . b_j             the LOWEST i among equal scores; a zero column scores 0 and may win
 *   c'_j    = x_{i*_j} . b_j                 (float32 fma in channel order, recomputed: not the search's score)
 *   E_cov   = (2/M) sum_j (1 - c'_j)
 *   S_cov,i = -(n/M) sum_{j : i*_j = i} (b_j - c'_j x_i) / r_i     (0 for r_i = 0; n d(E_cov/2)/df_i, winners held;
 *                                                                   rows added in ascending j)
 *   E = E_fwd + lambda E_cov,  S = S_fwd + lambda S_cov
 *   loss += lw w E / 2,  diff[layer] += lw w S / (sum|S| / (C n) + EPS)          (ONE normalisation, of the sum)
 * Zero bank rows count in M: each adds 1 to the sum and nothing to S.  The term belongs to one tile: every tile is
 * asked to cover the whole bank.  cover 0 is stx_set_nnfm_knn_targets, byte for byte; a cover that is negative or
 * not finite, or one other than 0 with patch 3 (the coverage part has no patch form), is STX_ERR_ARG.  Every other
 * refusal is that of stx_set_nnfm_knn_targets. */
typedef struct stx_nnfm_cover_target {
    const char *layer;
    int channels;
    int patch;
    int k;
    int rows;
    const float *bank;      /* [rows][patch * patch * channels] */
    int mem;
    double weight;
    float cover;
} stx_nnfm_cover_target;
/* stx_set_nnfm_targets for banks of any kind: a layer has ONE bank, and any of the four calls replaces the
 * whole set. */
int stx_set_nnfm_cover_targets(stx_engine *e, const stx_nnfm_cover_target *targets, int n);

/* The same term guided by regions ("semantic" style transfer: Champandard 2016, the guided forms of CNNMRF, STROTSS
 * and NNST): a column may only pick rows of the style picture whose region it lies in.  The bank of a layer is cut
 * into S segments, 1 <= S <= STX_NNFM_MAX_SEGMENTS; segment s holds the seg_rows[s] >= k unit rows of style picture
 * s, segment after segment.  Every segment has a mask, one [H][W] picture in the image frame of the current targets,
 * shared by every layer; the library keeps its block means at each layer's scale (the rule of stx_image_mask_map),
 * and m_s(i) in [0, 1] is the tile's window of that map, taken exactly like a content map's (start // s, roll // s,
 * wrapping, the same range error).  With r_i, x_i as above, for every segment s and column i:
 *   J_{i,s} = the k best rows OF SEGMENT s for x_i    (the order rule of stx_set_nnfm_knn_targets; indices local
 *                                                      to the segment)
 *   t_{i,s} = (1/k) sum_r b_{J_{i,s,r}}               (float32, rank order, then scaled)
 *   c_{i,s} = x_i . t_{i,s}                           (float32 fma in channel order, recomputed from (F, B, J))
 *   E   = (2/n) sum_i sum_s m_s(i) (1 - c_{i,s})
 *   S_i = sum_s m_s(i) ( -(t_{i,s} - c_{i,s} x_i) / r_i )        (segments added in ascending s; 0 for r_i = 0)
 *   a   = sum_i sum_s m_s(i) / n
 *   loss += lw w E / 2,  diff[layer] += lw w a S / (sum|S| / (C n) + EPS)
 * a plays the part it plays in stx_set_content_mask: the normalisation would otherwise undo the masks' overall
 * level.  Masks that partition the picture give a = 1; one segment with m = 1 is stx_set_nnfm_knn_targets byte for
 * byte; m = 0 everywhere adds nothing.  Query blocks are 128 consecutive columns of the blob in row-major order, and
 * segment s is searched for a block exactly when some column of the block has m_s > 0: with hard-edged masks that
 * partition the picture the search does about 1/S of the work over the whole bank.  For a pair that is not searched
 * no row of the segment is read.  No float atomics, every sum in a fixed order: the same inputs give the same bits.
 * Patch 1 and no coverage part only.  STX_ERR_ARG: segments outside 1 .. STX_NNFM_MAX_SEGMENTS, a segment with fewer
 * rows than k, k outside 1 .. 4, no masks or a bad mask size; every other refusal is that of stx_set_nnfm_targets. */
#define STX_NNFM_MAX_SEGMENTS 8
typedef struct stx_nnfm_guided_target {
    const char *layer;
    int channels;
    int k;
    int segments;
    const int *seg_rows;    /* [segments] (host) */
    const float *bank;      /* [sum of seg_rows][channels] */
    int mem;
    double weight;
} stx_nnfm_guided_target;
/* stx_set_nnfm_targets for guided banks: a layer has ONE bank, and any of the five calls replaces the whole set.
 * masks: `segments` pictures [H][W] (host pointers to host or device arrays, by mask_mem); every target has
 * `segments` segments. */
int stx_set_nnfm_guided_targets(stx_engine *e, const stx_nnfm_guided_target *targets, int n,
                                const float *const *masks, int segments, int H, int W, int mask_mem);

/* The sliced Wasserstein term (not in the reference): the loss of Heitz et al., "A Sliced Wasserstein Loss for
 * Neural Texture Synthesis" (CVPR 2021).  It holds the WHOLE distribution of a layer's feature vectors, not its
 * second moments (the Gram and statistics terms) and not single vectors (NNFM).  A tapped blob F [C][h][w] -- the
 * array the Gram term reads -- has n = h w columns f_i.  The caller gives D unit directions V [D][C] (float32) and
 * a target Tq [D][Q] (float32): per direction a non-decreasing quantile function, sampled at u_q = (q + 1/2) / Q.
 *   p[d][i]  = v_d . f_i                         (float32 accumulation; -0 counts as +0)
 *   r_d(i)   = rank of i when p[d][.] is ordered ascending, equal values by ascending i  (a strict total order)
 *   t[d][r]  = resample(Tq[d], Q -> n)[r]
 *   g[d][i]  = p[d][i] - t[d][r_d(i)]
 *   E        = (1/(D n)) sum_d sum_i g[d][i]^2
 *   S[c][i]  = (1/D) sum_d g[d][i] V[d][c]       ( = n d(E/2)/dF with the ranks held )
 *   loss        += lw weight E / 2
 *   diff[layer] += lw weight S / (sum|S| / (C n) + EPS)      (the reference's normalize, as for the Gram term)
 * resample(s[0 .. M-1], M -> K)[k] is one rule, in integer arithmetic, used here and in target making:
 *   1. num = (2 k + 1) M - K in int64;
 *   2. num <= 0: the result is s[0];
 *   3. otherwise j = num div 2 K and a = float32(num mod 2 K) / float32(2 K);
 *   4. j >= M - 1: the result is s[M - 1];
 *   5. otherwise the result is fma(a, s[j + 1] - s[j], s[j]).
 * With K = M this returns s[k] bit for bit.  A tile's term is the tile's own, as its Gram is.  No float atomics;
 * every sum is added in a fixed order, and the order above is total, so the sort's form does not show: the same
 * inputs give the same bits.  A blob whose targets are its own sorted projections (stx_swd_target with Q = n)
 * contributes exactly 0 to the loss and to the gradient.
 * (A struct tag only: stx_swd_target without `struct` is the function that makes a target, below.) */
struct stx_swd_target {
    const char *layer;
    int channels;
    int dirs;               /* D */
    int quantiles;          /* Q */
    const float *V;         /* [dirs][channels] */
    const float *Tq;        /* [dirs][quantiles] */
    int mem;
    double weight;
};
/* Replaces all sliced Wasserstein targets of the engine's group (n = 0: none); one per layer at most.  V and Tq
 * are copied.  They are shared like the style targets (stx_engine_create_shared) and
 * stx_set_contents_and_styles clears them: call this behind it.  A layer with a target is part of every
 * stx_sc_grad_tile evaluation under the rules of stx_set_stat_targets: the layer_weight of its tap if the tap
 * list names it, lw = 1 otherwise, and all layers on one path.  The term follows the blob's NNFM term in the loss
 * and in the gradient.  STX_ERR_ARG for a channel count other than the layer's, dirs < 1 or quantiles < 2;
 * STX_ERR_UNSUPPORTED for channels not a multiple of 4, dirs > 4096, quantiles > 65536 and -- at the evaluation --
 * a tile whose blob has n > 2^22 or dirs x (n padded to a power of two) >= 2^31. */
int stx_set_swd_targets(stx_engine *e, const struct stx_swd_target *targets, int n);

/* The self-similarity content term (not in the reference): the content loss of STROTSS (Kolkin et al., CVPR 2019;
 * NNST uses the same term).  The content term pins feature VALUES; this one holds the PATTERN of similarities
 * between positions -- two places that look alike in the content picture should look alike in the result, two that
 * differ should differ -- and leaves the features themselves free.  A tapped blob F [C][h][w] lies at a layer that
 * holds a content map of content_index 0; c is the tile's window of that map, the very window the content term
 * takes (start // s, roll // s, wrapping, the same range error).
 * The sample grid: g is the smallest integer >= 1 with ceil(h/g) ceil(w/g) <= points; the positions are (a g, b g)
 * in raster order, N = ceil(h/g) ceil(w/g) of them (--nnfm-stride's rule).  f_i is the column of F at position i,
 * c_i that of c.  All sums run in a fixed order.
 *   r_i   = |f_i|,  x_i = f_i / r_i            (r_i = 0: x_i = 0, 1/r_i = 0);   y_i likewise from c_i
 *   DX_ij = 1 - x_i . x_j  (i != j),  DX_ii = 0 exactly;                 DC likewise from y
 *   sX_j  = sum_i DX_ij + N 1e-6;                                        sC likewise
 *   PX_ij = DX_ij / sX_j,  PC_ij = DC_ij / sC_j          (every column a distribution of distances)
 *   d_ij  = PX_ij - PC_ij,  T_ij = sign(d_ij)  (sign(0) = 0)
 *   E     = (1/N) sum_ij |d_ij|                          (0 <= E <= 2)
 *   u_j   = sum_k T_kj PX_kj
 *   A_ij  = (T_ij - u_j) / sX_j  (i != j),  A_ii = 0
 *   q_i   = - sum_j (A_ij + A_ji) x_j
 *   S_i   = (q_i - (q_i . x_i) x_i) / (2 r_i)  at the sampled positions, 0 elsewhere   ( = N d(E/2)/d f_i, T held )
 *   loss        += lw weight E / 2
 *   diff[layer] += lw weight S / (sum|S| / (C h w) + EPS)      (the reference's normalize, as for every term)
 * The N 1e-6 is part of the definition: it keeps a tile of one colour (all y_i equal, DC at rounding noise)
 * well-defined.  N = 1 gives E = 0 and S = 0.  Both sides go through the same kernels in the same order, so a blob
 * that equals its window has d = 0 bit for bit and changes no bit of the loss or of the gradient.  D is formed in
 * float32 (float32 products, float32 accumulation): T is the sign of a difference of nearly equal numbers wherever
 * result and content agree.  No float atomics; the same inputs give the same bits. */
struct stx_selfsim_target {
    const char *layer;
    int points;             /* the most grid positions, 2 .. 4096 */
    double weight;
};
/* Replaces all self-similarity targets of the engine's group (n = 0: none); one per layer at most.  A target
 * carries no data of its own: the term reads the layer's content map of content_index 0, and a layer that holds
 * none is STX_ERR_ARG here.  The targets are shared like the style targets (stx_engine_create_shared) and
 * stx_set_contents_and_styles clears them: call this behind it.  A layer with a target is part of every
 * stx_sc_grad_tile evaluation under the rules of stx_set_stat_targets: the layer_weight of its tap if the tap list
 * names it, lw = 1 otherwise, and all layers on one path; whether the tap says is_content does not matter.  The
 * term follows the blob's SWD term in the loss and in the gradient.  STX_ERR_ARG for points outside 2 .. 4096;
 * STX_ERR_UNSUPPORTED for a layer whose channel count is not a multiple of 64. */
int stx_set_selfsim_targets(stx_engine *e, const struct stx_selfsim_target *targets, int n);

/* The shifted-Gram style term (not in the reference): the long-range statistic of Berger & Memisevic,
 * "Incorporating long-range consistency in CNN-based texture generation" (ICLR 2017).  The Gram, statistics and SWD
 * terms read a layer's feature vectors as a bag and NNFM reads 3 x 3 patches at most; this term holds the Gram
 * matrix of a blob against a copy of itself translated by delta pixels to the style picture's, for a list Delta of
 * offsets delta = (dy, dx), each along one axis: (0, d) or (d, 0), d >= 1.  A tapped blob F [C][h][w] -- the array
 * the Gram term reads -- with n = h w; per offset P_d = {p : p and p + delta both in the map}, n_d = (h - dy)(w - dx):
 *   X_d[a][b] = (1 / (C n_d)) sum_{p in P_d} F_a(p) F_b(p + delta)          full C x C, not symmetric
 *   D_d       = X_d - T_d                                                   T_d: the target, [C][C]
 *   E         = (1/|Delta|) sum_d sum_ab D_d[a][b]^2
 *   S_a(p)    = (1/|Delta|) sum_d (n / n_d) [ sum_b D_d[a][b] F_b(p + delta) [p + delta in the map]
 *                                           + sum_b D_d[b][a] F_b(p - delta) [p - delta in the map] ]
 *                                                                           ( = C n d(E/2)/dF_a(p), exactly )
 *   loss        += lw weight E / 2
 *   diff[layer] += lw weight S / (sum|S| / (C n) + EPS)      (the reference's normalize, as for every term)
 * The mean is over pairs (1 / n_d), so a style picture and a tile of different sizes have comparable X.  A tile's
 * term is the tile's own, as its Gram is: pairs across a tile edge are not counted.  C is a multiple of 32
 * (STX_ERR_UNSUPPORTED otherwise), 1 <= |Delta| <= 16; an offset that leaves an evaluated tile blob without a pair
 * (n_d < 1) is STX_ERR_ARG at the evaluation, before any launch, and the message names the layer and the offset.
 * No atomics; partial sums are added in a fixed order: the same inputs give the same bits.  X_d is rounded to
 * float32 once and D, E and S are formed from the rounded values: a tile whose X_d equal the targets (those
 * stx_shift_gram gives for the same array) contributes exactly 0 to the loss and changes no bit of the gradient. */
struct stx_shift_target {
    const char *layer;
    int channels;
    int n_offsets;          /* |Delta|, 1 .. 16 */
    const int *offsets;     /* host, [n_offsets][2] = dy, dx */
    const float *grams;     /* T, [n_offsets][channels][channels] */
    int mem;                /* of grams */
    double weight;
};
/* Replaces all shifted-Gram targets of the engine's group (n = 0: none); one per layer at most.  They are shared
 * like the style targets (stx_engine_create_shared) and stx_set_contents_and_styles clears them: call this behind it.
 * A channel count other than the layer's is STX_ERR_ARG here.  A layer with a target is part of every
 * stx_sc_grad_tile evaluation under the rules of stx_set_stat_targets: the layer_weight of its tap if the tap list
 * names it, lw = 1 otherwise, an empty tap list accepted, and all layers on one path.  The term follows the blob's
 * self-similarity term in the loss and in the gradient. */
int stx_set_shift_targets(stx_engine *e, const struct stx_shift_target *targets, int n);

/* The contextual style term (not in the reference): the contextual loss of Mechrez, Talmi, Zelnik-Manor, "The
 * Contextual Loss for Image Transformation with Non-Aligned Data" (ECCV 2018).  The Gram, statistics, SWD and
 * shifted-Gram terms hold global statistics and the NNFM family takes hard nearest neighbours; this term matches
 * softly and free of scale: each sampled feature vector of the result spreads a softmax over the whole style bank
 * at a temperature that follows its own best distance, and each bank row is credited with the best share any
 * vector gives it.  A tapped blob F [C][h][w]; the sample grid is that of stx_set_selfsim_targets: g the smallest
 * integer >= 1 with ceil(h/g) ceil(w/g) <= points, positions (a g, b g) in raster order, N of them, columns f_i.
 * The bank is built once per target from raw style rows y_k [M][C] (stx_cx_bank):
 *   mu = (1/M) sum_k y_k,   b_k = (y_k - mu) / |y_k - mu|       (zero where the norm is 0; sums in double)
 * and with eps = 1e-5, eta = h (the bandwidth), all sums in a fixed order:
 *   z_i  = f_i - mu,  r_i = |z_i|,  x_i = z_i / r_i              (r_i = 0: x_i = 0, 1/r_i = 0)
 *   s_ik = x_i . b_k                                             (float32 products, float32 accumulation)
 *   k*_i = argmax_k s_ik (the LOWEST k among equal scores),  a_i = 1 - s_{i,k*_i},  tau_i = eta (a_i + eps)
 *   e_ik = exp((s_ik - s_{i,k*_i}) / tau_i),  Z_i = sum_k e_ik,  p_ik = e_ik / Z_i,  u_i = sum_k p_ik s_ik
 *   i*_k = argmax_i p_ik (the LOWEST i among equal values),  m_k = p_{i*_k,k}
 *   CX   = (1/M) sum_k m_k,   E = -log CX                        (E >= 0; N = M = 1 gives E = 0, S = 0)
 *   P_i  = sum_{k: i*_k = i} p_ik,   Q_i = sum_{k: i*_k = i} p_ik s_ik
 *   g_ik = -(1/(M CX)) [ p_ik (1[i*_k = i] - P_i) / tau_i  +  1[k = k*_i] eta (Q_i - P_i u_i) / tau_i^2 ]
 *   q_i  = sum_k g_ik b_k
 *   S_i  = (q_i - (q_i . x_i) x_i) / r_i  at the grid positions, 0 elsewhere    ( = dE/df_i with k*, i* held )
 *   loss        += lw weight E                                   (E whole: it is no half square)
 *   diff[layer] += lw weight S / (sum|S| / (C h w) + EPS)        (the reference's normalize, as for every term)
 * p_ik is the paper's CX_ij: its exp((1 - d~) / h) differs from e_ik by a factor that cancels in the row
 * normalisation, and the form above cannot overflow.  The second part of g is the derivative through the row
 * minimum.  Two identical columns f_i tie exactly in i*, and E has a kink there.  A tile's term is the tile's own:
 * every tile's sample is asked to cover the whole bank, as with stx_set_nnfm_cover_targets.  exp is the accurate
 * expf.  No atomics, no scratch memory; every sum in a fixed order: the same inputs give the same bits. */
struct stx_cx_target {
    const char *layer;
    int channels;
    int rows;               /* M, 1 .. 16384 */
    const float *raw_rows;  /* y, [rows][channels]: raw feature vectors (stx_cx_rows), not normalised */
    int mem;                /* of raw_rows */
    int points;             /* the most grid positions, 2 .. 4096 */
    double h;               /* the bandwidth eta, > 0 */
    double weight;
};
/* Replaces all contextual targets of the engine's group (n = 0: none); one per layer at most.  The rows are copied
 * and mu and the bank are built here.  The targets are shared like the style targets (stx_engine_create_shared)
 * and stx_set_contents_and_styles clears them: call this behind it.  A layer with a target is part of every
 * stx_sc_grad_tile evaluation under the rules of stx_set_stat_targets: the layer_weight of its tap if the tap list
 * names it, lw = 1 otherwise, an empty tap list accepted, and all layers on one path.  The term follows the blob's
 * shifted-Gram term in the loss and in the gradient.  STX_ERR_ARG for a channel count other than the layer's,
 * points outside 2 .. 4096, rows outside 1 .. 16384, h <= 0 or not finite; STX_ERR_UNSUPPORTED for channels not a
 * multiple of 64 and for points x rows > 2^24 (the two N x M matrices exist in memory). */
int stx_set_cx_targets(stx_engine *e, const struct stx_cx_target *targets, int n);

/* --------------------------------------------------------------------------- the hot path */
/* Replaces CaffeModel.eval_features_tile via FeatureMapRequest (style_transfer.py:156,221-228,
 * 421-427): forward the tile and return the post-ReLU maps of the requested blobs.
 * out[i] receives [C_i][ceil(th/scale_i)][ceil(tw/scale_i)] floats. */
int stx_features_tile(stx_engine *e, const float *img, int img_mem, int th, int tw,
                      const char *const *layers, int n_layers, float *const *out, int out_mem);

/* One tapped blob of an SCGradRequest: layer_weights[layer], content_weight[layer] (0 = not a
 * content layer), style_weight[layer] (0 = not a style layer) -- style_transfer.py:158-161,570,
 * 579-580,591-593 -- and dd_weight[layer] (0 = not a Deep-Dream layer): loss -= lw*dd*1/2|F|^2,
 * diff -= lw*dd*normalize(F), style_transfer.py:602-604. */
typedef struct stx_tap {
    const char *layer;
    double layer_weight;
    int is_content;
    double content_weight;
    int is_style;
    double style_weight;
    int is_dd;
    double dd_weight;
} stx_tap;

/* Replaces the SCGradRequest branch of TileWorker.process_one_request + CaffeModel.
 * eval_sc_grad_tile (style_transfer.py:230-241,556-612).
 *   img        [3][th][tw] tile of the (rolled) image;
 *   roll_xy    the request's roll: the engine addresses its content maps as if rolled by
 *              roll_xy // scale with numpy.roll(axis=(-1,-2)) semantics, i.e. roll_xy[0] shifts
 *              the W axis and roll_xy[1] the H axis (num_utils.py:136-140); no copy is made;
 *   start_yx   tile origin in the rolled image (y, x) (style_transfer.py:571-573);
 *   loss_out   host double; written by the next stx_sync() (or immediately if sync_now != 0);
 *   grad_out   [3][th][tw], the reference's diff['data'].
 * img is read and grad_out written in stream order on the engine's stream, where they are if they are
 * distinct STX_DEVICE buffers of the engine's own GPU that the first and the last kernel of the graph can
 * work on, through a copy otherwise; img is never written.  Both stay allocated until the
 * call has run.
 */
int stx_sc_grad_tile(stx_engine *e, const float *img, int img_mem, int th, int tw,
                     const int roll_xy[2], const int start_yx[2], const stx_tap *taps, int n_taps,
                     double *loss_out, float *grad_out, int grad_mem, int sync_now);

/* Zero-copy hand-off for callers that produce the tile on the engine's own GPU (the tile farm
 * cuts tiles with stx_image_cut_tile): *tile_in is the engine's input blob sized for a
 * [3][th][tw] tile, *grad_out the blob its gradient is left in.  Passing exactly these pointers
 * as `img` / `grad_out` of stx_sc_grad_tile (same th, tw) skips the two device-to-device copies
 * of the call.  The pointers are valid until a larger tile is evaluated on this engine: query
 * them again before every use.  (The reference copies every tile into and out of POSIX shared
 * memory, style_transfer.py:634-643.) */
int stx_tile_buffers(stx_engine *e, int th, int tw, float **tile_in, float **grad_out);

/* Lower-triangular Gram of a feature map, F F^T / (C*h*w), upper triangle zero: gram_matrix
 * (num_utils.py:143-147) as used for the style targets (style_transfer.py:534). */
int stx_gram_matrix(stx_engine *e, const float *feat, int feat_mem, int channels, int hw,
                    float *gram_out, int gram_mem);

/* Per-channel mean and sd = sqrt(population variance + 1e-5) of a feature map [channels][hw], as float32:
 * what stx_set_stat_targets takes, by the launches the term itself runs on a tile's blob. */
int stx_feature_stats(stx_engine *e, const float *feat, int feat_mem, int channels, int hw,
                      float *mean_out, float *sd_out, int out_mem);

/* The sliced Wasserstein target of a feature map [channels][h][w] along `dirs` directions V [dirs][channels]
 * (stx_set_swd_targets): the projections as the term forms them, each direction's M = h w values sorted, and
 * out [dirs][quantiles] = resample(sorted, M -> quantiles); with quantiles = M the sorted projections
 * themselves.  V and out are STX_HOST; synchronous.  Refusals: those of the term. */
int stx_swd_target(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, const float *V,
                   int dirs, int quantiles, float *out);

/* The shifted Grams X_d of a feature map [channels][h][w] for the offsets [n_offsets][2] = dy, dx (host): what
 * stx_set_shift_targets takes, by the launches the term itself runs on a tile's blob.  out [n_offsets][channels]
 * [channels] is STX_HOST; synchronous.  Refusals: those of the term. */
int stx_shift_gram(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, const int *offsets,
                   int n_offsets, float *out);

/* The raw rows of a feature map [channels][h][w] for a contextual bank (stx_set_cx_targets): its columns on the
 * grid of a budget of `rows` positions (the rule of the term's sample grid), in raster order, as float32 rows
 * [N][channels], N = ceil(h / g) ceil(w / g) <= rows, bit for bit.  Rows of several pictures are concatenated by
 * the caller.  rows < 1 is STX_ERR_ARG; channels not a multiple of 64 (the term's own limit): STX_ERR_UNSUPPORTED,
 * before any launch. */
int stx_cx_rows(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int rows, float *rows_out,
                int out_mem);
/* mu [channels] and the centred unit rows bank [rows][channels] of raw rows [rows][channels], as
 * stx_set_cx_targets builds them: column sums and norms in double in a fixed order.  Synchronous.  Channels not a
 * multiple of 64: STX_ERR_UNSUPPORTED; rows outside 1 .. 16384: STX_ERR_ARG. */
int stx_cx_bank(stx_engine *e, const float *raw_rows, int mem, int channels, int rows, float *mu_out, float *bank_out,
                int out_mem);

/* The NNFM bank of a feature map [channels][h][w]: its unit-normalised columns at (y, x) with y % stride == 0
 * and x % stride == 0, in raster order, as float32 rows [rows][channels], rows = ceil(h / stride) *
 * ceil(w / stride).  A zero column stays as a zero row.  Banks of several pictures are concatenated by the
 * caller.  By the pass that prepares a tile's blob for the search. */
int stx_nnfm_bank(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int stride,
                  float *bank_out, int out_mem);
/* patch 3: the unit patches (stx_set_nnfm_patch_targets) centred at those (y, x), [rows][9 channels]; an
 * all-zero patch stays a zero row.  The stride thins the centres only: a patch takes its eight neighbours at
 * distance one in the full map.  patch 1: stx_nnfm_bank. */
int stx_nnfm_patch_bank(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int patch,
                        int stride, float *bank_out, int out_mem);

/* ------------------------------------------------- full-image ops (device-resident state) */
/* All pointers in this group are STX_DEVICE memory on the engine's GPU, images are [3][H][W].
 * The image and the optimizer state are kept UN-rolled; the per-iteration random shift
 * (style_transfer.py:777-806) is applied as an index offset when tiles are cut and when tile
 * gradients are put back, which is equivalent to the reference's roll / un-roll pair. */

/* tile[c][y][x] = img[c][(y0 + y - roll_xy[1]) mod H][(x0 + x - roll_xy[0]) mod W]: the window
 * [y0,y0+th) x [x0,x0+tw) of roll2(img, roll_xy) (style_transfer.py:632,661). */
int stx_image_cut_tile(stx_engine *e, const float *img, int H, int W, const int roll_xy[2],
                       int y0, int x0, int th, int tw, float *tile);
/* Inverse placement of a tile gradient into the un-rolled full gradient
 * (style_transfer.py:642 followed by the un-roll at 805-806). */
int stx_image_put_tile(stx_engine *e, float *grad, int H, int W, const int roll_xy[2],
                       int y0, int x0, int th, int tw, const float *tile_grad);

/* Feature-map preprocessing on the device (eval_features_once / prepare_features,
 * style_transfer.py:429-486), so that per-scale targets never visit the host:
 * stx_map_place puts one tile's [C][h][w] map into the full-image map [C][dst_h][dst_w] at
 * (y0, x0) (the stitch at style_transfer.py:457-461); stx_map_roll_add does one pass of the
 * rolled-tiling average (style_transfer.py:476-485) on [C][h][w] maps:
 * init_divisor != 0:  acc  = roll2(src, roll_xy) / init_divisor   (features = feats / passes)
 * init_divisor == 0:  acc += alpha * roll2(src, roll_xy)          (saxpy(1 / passes, ...)) */
/* One layer's mask map (stx_set_style_masks): out [ceil(H/scale)][ceil(W/scale)] = block means of mask. */
int stx_image_mask_map(stx_engine *e, const float *mask, int H, int W, int scale, float *out);
int stx_map_place(stx_engine *e, float *dst, int channels, int dst_h, int dst_w, int y0, int x0,
                  const float *src, int h, int w);
int stx_map_roll_add(stx_engine *e, float *acc, const float *src, int channels, int h, int w,
                     const int roll_xy[2], double alpha, double init_divisor);

/* Resampling between pyramid scales (num_utils.resize, num_utils.py:90-108, used by
 * style_transfer.py:399-401 and optimizers.py:53-61): Pillow's separable 'F'-mode resampler --
 * horizontal pass, then vertical pass on the float32 intermediate, double accumulation.  The
 * caller supplies, per axis, the window table bounds[out][2] = (first input index, tap count) and
 * the normalised weights[out][ksize] (host memory); src [C][H][W] and dst [C][out_h][out_w] are
 * STX_DEVICE.  clamp_min_zero applies max(0, .) to the result (the Adam g2 state).  Synchronous. */
int stx_image_resample(stx_engine *e, const float *src, int channels, int H, int W, float *dst,
                       int out_h, int out_w, const int *bounds_x, const double *weights_x,
                       int ksize_x, const int *bounds_y, const double *weights_y, int ksize_y,
                       int clamp_min_zero);

/* TV + p-norm + auxiliary-image terms of eval_loss_and_grad (style_transfer.py:709-733,
 * num_utils.py:74-82,150-162): grad += tv_scale*d tv_norm(img/127.5, tv_power)
 *                                    + p_scale*d p_norm((img+mean-127.5)/127.5, p_power)
 *                                    + aux_scale*(img-aux')/127.5;
 * *loss_out (host, written at stx_sync) = tv_scale*TV + p_scale*P + aux_scale*A.
 * A scale of 0 disables a term; aux may be NULL.  mean_bgr is a host array of 3 floats.
 * aux_roll_xy (or NULL = no shift): the reference rolls the image by the iteration's shift but
 * not its auxiliary image (style_transfer.py:729-733,777-786), so in the un-rolled frame used here
 * aux'[y][x] = aux[(y + roll_xy[1]) mod H][(x + roll_xy[0]) mod W]. */
int stx_image_regularizers(stx_engine *e, const float *img, float *grad, int H, int W,
                           const float mean_bgr[3], double tv_scale, double tv_power,
                           double p_scale, double p_power, const float *aux, double aux_scale,
                           const int aux_roll_xy[2], double *loss_out);

/* The SWT term of eval_loss_and_grad (style_transfer.py:716-720, num_utils.py:179-196) for the
 * reference's defaults --swt-wavelet haar --swt-levels 1:
 *   D = detail part (approximation band zeroed) of the one-level stationary Haar transform of
 *       roll(img)/127.5, taken on its symmetric padding to a power-of-two square and cropped back;
 *   grad += scale * d p_norm(D, power) (the p-norm's own gradient at D, as the reference adds it);
 *   *loss_out (host, written at stx_sync) = scale * sum |D|^power.
 * roll_xy (or NULL): the iteration's shift; the image itself stays un-rolled.  PyWavelets is not
 * part of the reference tree: the transform is restated (oracle/num_ops.py), parity unpinned. */
int stx_image_swt_haar(stx_engine *e, const float *img, float *grad, int H, int W,
                       const int roll_xy[2], double scale, double power, double *loss_out);

/* The same term for --swt-levels L >= 1 of the Haar wavelet (style_transfer.py:716-720 passes the
 * level count to pywt.swt2 / iswt2 through num_utils.py:179-196).  Level j uses the two-tap filters
 * dilated by 2^(j-1), periodic on the padded N x N square; with every approximation band zeroed the
 * inverse drops the path through the deepest approximation band alone, which leaves
 *   D = x - B_L x,  B_L = T_L along rows x T_L along columns,  T_L[k] = (2^L - |k|) / 4^L, |k| < 2^L
 * (the product over j of [1 2 1]/4 at stride 2^(j-1)), x = roll(img)/127.5 padded symmetrically.
 * grad, *loss_out and roll_xy are those of stx_image_swt_haar; asynchronous like it.
 * levels < 1 or levels > log2(N), N = 2^ceil(log2(max(H, W))), is STX_ERR_ARG (PyWavelets refuses
 * such a count too).  levels == 1 runs stx_image_swt_haar itself: bit-identical results. */
int stx_image_swt_haar_levels(stx_engine *e, const float *img, float *grad, int H, int W, int levels,
                              const int roll_xy[2], double scale, double power, double *loss_out);

/* The same term for --swt-wavelet dbN / symN: `order` = N vanishing moments, 1..38 (PyWavelets' db
 * range; symN exists for N = 2..20).  An orthonormal bank's shift-averaged inverse is half the
 * adjoint per level and axis, so zeroing the approximation bands leaves, as for Haar,
 *   D = x - B_L x,  B_L per axis = product over j = 1..L of (r/2 at stride 2^(j-1)),
 * r the autocorrelation of the low-pass filter.  r depends on |H|^2 alone, which dbN and symN share
 * (one call serves both): the maximally flat half-band filter, r[0] = 1, r[+-(2k-1)] =
 * prod over m != k of (1/2 - m)/(k - m), m, k = -N+1..N, zero at the other even offsets
 * (N = 1: [1/2 1 1/2], the triangle above; N = 2: [-1/16 0 9/16 1 9/16 0 -1/16]).  The library
 * builds the taps of B_L in double, folds them onto the periodic padded square, rounds them to
 * float once and keeps them on the device per (order, levels, padded side): only the first call
 * with a new triple uploads (and synchronises for) anything.  Parity with PyWavelets is unpinned
 * as for Haar (the package is in neither tree).
 * Everything else -- grad, *loss_out, roll_xy, padding, asynchrony, the level check -- is
 * stx_image_swt_haar_levels'.  order outside 1..38 is STX_ERR_ARG.  order == 1 runs
 * stx_image_swt_haar_levels itself: bit-identical results. */
int stx_image_swt_daub_levels(stx_engine *e, const float *img, float *grad, int H, int W,
                              int order, int levels, const int *roll_xy,
                              double scale, double power, double *loss_out);

/* AdamOptimizer.update after the gradient is known (optimizers.py:35-42), fused:
 *   g1 = b1*g1 + (1-b1)*grad; g2 = b2*g2 + (1-b2)*grad^2; p1 likewise on the new params;
 *   params -= lr * (g1/c1) / (sqrt(g2/c2) + EPS);  avg_out = p1/cp
 * where c1, c2, cp are the EWMA bias corrections (1 - beta^t, or 1 when uncorrected).
 * n == 0 is STX_ERR_ARG, here and in every stx_vec_* call below: nothing is launched. */
int stx_adam_step(stx_engine *e, float *params, const float *grad, float *g1, float *g2, float *p1,
                  float *avg_out, size_t n, double lr, double b1, double b2, double bp1,
                  double corr1, double corr2, double corrp);

/* BLAS-1 pieces of LBFGSOptimizer (optimizers.py:74-121; num_utils.py:20-42). */
int stx_vec_dot(stx_engine *e, const float *x, const float *y, size_t n, double *out_host_sync);
int stx_vec_axpy(stx_engine *e, double a, const float *x, float *y, size_t n);
int stx_vec_scale(stx_engine *e, double a, float *x, size_t n);
int stx_vec_mean_abs(stx_engine *e, const float *x, size_t n, double *out_host_sync);
/* The same recursion with its scalars kept on the device (no host round trip per dot product;
 * LBFGSOptimizer.inv_hv, optimizers.py:105-121).  *_dev arguments point to STX_DEVICE doubles.
 *   stx_vec_dot_async:      *out_dev = <x, y>            stx_vec_abs_sum_async: *out_dev = sum |x|
 *   stx_vec_axpy_dev:       y += (float)(*a_dev / da * c1 [+ *b_dev / db * c2]) * x   (b_dev may be NULL)
 *   stx_vec_scale_dev:      x *= (float)(c / (*den_dev / den_div))
 * All asynchronous, ordered on the engine stream. */
int stx_vec_dot_async(stx_engine *e, const float *x, const float *y, size_t n, double *out_dev);
int stx_vec_abs_sum_async(stx_engine *e, const float *x, size_t n, double *out_dev);
int stx_vec_axpy_dev(stx_engine *e, double c1, const double *a_dev, double da, double c2,
                     const double *b_dev, double db, const float *x, float *y, size_t n);
int stx_vec_scale_dev(stx_engine *e, double c, const double *den_dev, double den_div, float *x,
                      size_t n);
/* Fused passes of the same step (round 5): each computes, value for value and bit for bit, what the
 * separate calls above compute, and reads an array once where they read it two or three times.
 *   stx_vec_axpy_dot_dev:   y = coef * x + src (coef as stx_vec_axpy_dev; src may be y); with scale_den_dev
 *                           != NULL then y *= (float)(scale_c / (*scale_den_dev / scale_div)); *out_dev =
 *                           <z, y> -- the axpy of one iteration of inv_hv's loops (and the scaling between
 *                           them) with the dot product of the next (optimizers.py:108-120)
 *   stx_vec_lbfgs_pair:     y = g_new - g_old, g_old = g_new, out_dev2[0] = <s, y>, out_dev2[1] = <y, y>;
 *                           *sy_host_sync = out_dev2[0] after a stream synchronisation -- the curvature
 *                           pair and its test (optimizers.py:84-85,97-103)
 *   stx_vec_scale2_axpy:    s = c2 * (c1 * s), params += s        (optimizers.py:76-82)              */
int stx_vec_axpy_dot_dev(stx_engine *e, double c1, const double *a_dev, double da, double c2,
                         const double *b_dev, double db, double scale_c, const double *scale_den_dev,
                         double scale_div, const float *x, const float *src, float *y, const float *z,
                         size_t n, double *out_dev);
int stx_vec_lbfgs_pair(stx_engine *e, const float *g_new, float *g_old, const float *s, float *y, size_t n,
                       double *out_dev2, double *sy_host_sync);
int stx_vec_scale2_axpy(stx_engine *e, double c1, double c2, float *s, float *params, size_t n);

/* Per-step statistics of transfer() (style_transfer.py:808-815):
 * stats[0] = mean|avg - old|, stats[1] = sqrt(mean(xdiff^2 + ydiff^2)) with circular forward
 * differences; then old <- avg.  Synchronous (returns after the values are on the host). */
int stx_image_step_stats(stx_engine *e, const float *avg, float *old, int H, int W,
                         double stats[2]);
/* The same kernel without the host wait: raw_sums[0] = sum|avg - old|, raw_sums[1] = sum(xdiff^2 +
 * ydiff^2) over the 3*H*W elements are written (host doubles) when the engine's pending values are
 * published -- stx_sync, or stx_fence_wait on a later fence; the caller divides by 3*H*W and
 * takes the root (style_transfer.py:808-812). */
int stx_image_step_stats_async(stx_engine *e, const float *avg, float *old, int H, int W,
                               double raw_sums[2]);

/* get_image (style_transfer.py:378-386): out_rgb_u8[H][W][3] = uint8(clip(img + mean, 0, 255))
 * with BGR->RGB flip and truncation toward zero.  out is STX_DEVICE memory. */
int stx_image_to_u8(stx_engine *e, const float *img, int H, int W, const float mean_bgr[3],
                    uint8_t *out_rgb_u8);

/* Colour-preserving transfer (Gatys et al., "Preserving Color in Neural Artistic Style Transfer").
 * Pictures are [3][H][W] float32 STX_DEVICE arrays in the network's input format: BGR planes with
 * mean_bgr subtracted.
 *   stx_image_to_u8_luma:   the luminance of img on the chroma of content.  Per pixel and channel
 *                           x = clip(img + mean, 0, 255), c = clip(content + mean, 0, 255), Y(v) =
 *                           0.299 v_R + 0.587 v_G + 0.114 v_B; out = uint8(clip(c + (Y(x) - Y(c)), 0,
 *                           255)), RGB HWC and truncated like stx_image_to_u8 (which it equals when
 *                           content == img).  One pass.
 *   stx_image_color_stats:  out_host_sync = the three channel sums (b, g, r) and the six distinct
 *                           second-moment sums (bb, bg, br, gg, gr, rr) of the stored values: float
 *                           per-block partials added in double in a fixed order -- the same input
 *                           gives the same nine doubles.  Synchronous, like stx_image_step_stats.
 *   stx_image_color_affine: dst_i = clip(sum_j A[3 i + j] src_j + b[i] + mean[i], 0, 255) - mean[i];
 *                           dst may be src.  A and b are used as float32.                          */
int stx_image_to_u8_luma(stx_engine *e, const float *img, const float *content, int H, int W,
                         const float mean_bgr[3], uint8_t *out_rgb_u8);
int stx_image_color_stats(stx_engine *e, const float *img, int H, int W, double out_host_sync[9]);
int stx_image_color_affine(stx_engine *e, const float *src, float *dst, int H, int W, const double A[9],
                           const double b[3], const float mean_bgr[3]);

/* The Laplacian loss (Li, Xu, Nie, Liu, "Laplacian-Steered Neural Style Transfer", 2017): holds the
 * iterate to the edges of a content picture.  Pictures are [3][H][W] float32 STX_DEVICE arrays, BGR
 * planes with the mean subtracted, un-rolled; the term ignores the iteration's shift.  For a pool
 * size p:
 *   u(x)  = (x_B + x_G + x_R) / 382.5
 *   P_p u = block means over p x p blocks from the picture's origin: hp x wp = ceil(H / p) x
 *           ceil(W / p) cells, edge cells over the pixels that exist
 *   D v   = sum over the 4-neighbours n inside the grid of (v - v_n)   ([0 -1 0; -1 4 -1; 0 -1 0]
 *           with a replicated border: symmetric, and zero on constants, so the mean never enters)
 *   T_p   = D P_p u(content),   e_p = D P_p u(img) - T_p
 *   loss  = scale * sum_p weights[p] * sum_cells e_p^2
 *   grad[ch][y][x] += scale * sum_p weights[p] * 2 (D e_p)[y / p][x / p] / (n_cell * 382.5), every ch
 * pools: n_pools = 1..4 distinct powers of two in 1..64; anything else, or a null pointer, is
 * STX_ERR_ARG.  The image is read once whatever n_pools is, and the gradient is read and written
 * once: the per-pixel sum over the sizes is formed first and added to each plane in one float32
 * addition (pixels whose sum is zero are not touched).  The target and the image run through the
 * same device code: img == content gives a loss of exactly 0 and leaves grad as it is.  No atomics:
 * the same inputs give the same bits.
 *   stx_image_lap_floats:  floats of a target = sum over pools of hp * wp (0 on a bad argument)
 *   stx_image_lap_target:  target_out (STX_DEVICE) = [T_p for p in pools], map after map; asynchronous
 *   stx_image_lap:         *loss_out (host) is written at the next stx_sync; asynchronous like
 *                          stx_image_regularizers.  target: what stx_image_lap_target left for the
 *                          same H, W and pools. */
size_t stx_image_lap_floats(int H, int W, int n_pools, const int *pools);
int stx_image_lap_target(stx_engine *e, const float *content, int H, int W, int n_pools,
                         const int *pools, float *target_out);
int stx_image_lap(stx_engine *e, const float *img, float *grad, int H, int W, int n_pools,
                  const int *pools, const double *weights, const float *target, double scale,
                  double *loss_out);

/* The photorealism regulariser (Luan, Paris, Shechtman, Bala, "Deep Photo Style Transfer", 2017): the
 * quadratic form of the matting Laplacian (Levin, Lischinski, Weiss) of a content picture, matrix-free.
 * It is zero where the iterate is locally an affine function of the content picture's colours.
 * Pictures are [3][H][W] float32 STX_DEVICE arrays, un-rolled; the term ignores the iteration's shift.
 * With I = content / 255 (a 3-vector per pixel), v = a plane of img / 255 and the 3 x 3 windows w_k
 * centred on the interior pixels (1 <= y <= H - 2, 1 <= x <= W - 2):
 *   mu_k = mean_w I,  m_k = mean_w v,  S_k = mean_w (I - mu_k)(I - mu_k)^T,  q_k = mean_w (I - mu_k)(v - m_k)
 *   a_k  = (S_k + (eps / 9) Id)^-1 q_k
 *   r_ki = (v_i - m_k) - a_k . (I_i - mu_k)                     for the nine pixels i of w_k
 *   loss = scale * sum over planes and windows of [ sum_i r_ki^2 + eps |a_k|^2 ]
 *   grad[c][i] += scale * 2 * (sum over the windows k that hold i of r_ki) / 255
 * A corner pixel is in one window, an interior pixel in nine.  Everything between the float32 pictures
 * and the float32 gradient is float64 on the device; the sum of a pixel is formed first, rounded to
 * float32 and added once: grad is read and written once.  Nothing is kept between calls.  No atomics:
 * the same inputs give the same bits.  A null pointer, H < 3, W < 3 or an eps that is not finite and
 * positive is STX_ERR_ARG.  *loss_out (host) is written at the next stx_sync; asynchronous like
 * stx_image_lap. */
int stx_image_photo(stx_engine *e, const float *img, const float *content, float *grad, int H, int W,
                    double eps, double scale, double *loss_out);

/* The temporal-consistency term for video (Ruder, Dosovitskiy, Brox, "Artistic Style Transfer for
 * Videos", 2016): earlier stylised frames, warped to the current frame by optical flow and composited,
 * hold the iterate wherever the flow is reliable.  All arrays are STX_DEVICE float32: pictures
 * [3][H][W] in the network's input format, un-rolled; flows [2][H][W], plane 0 horizontal and plane 1
 * vertical; weight [H][W].
 *
 * stx_image_flow_warp composites ONE earlier frame `prev` into target / weight.  flow_b is the backward
 * flow (current frame -> that frame), flow_f the forward flow (that frame -> current) or NULL; (su, sv)
 * scale the flows' components to pixels of this H x W (a flow resampled from W0 x H0: su = W / W0, sv =
 * H / H0).  Every value between the float32 inputs and outputs is float64 on the device, each operation
 * rounded once in the order written here.  For pixel (x, y):
 *   u = su * flow_b[0][y][x],  v = sv * flow_b[1][y][x]
 *   unknown     a flow vector with a component that is not finite or above 1e9 in magnitude BEFORE
 *               scaling (Middlebury's marker)
 *   q           = (x + u, y + v);   inside: 0 <= qx <= W - 1 and 0 <= qy <= H - 1
 *   taps        x0 = min(floor(qx), W - 2), fx = qx - x0;  y0, fy likewise
 *   mix(p)      = top + fy * (bottom - top),  top = p[y0][x0] + fx * (p[y0][x0+1] - p[y0][x0]),
 *               bottom the same on row y0 + 1;   value = mix(prev plane), per plane
 *   forward     (fu, fv) = (su * mix(flow_f[0]), sv * mix(flow_f[1])); an unknown vector at any of the
 *               four taps makes the pixel unreliable
 *   consistent  (u + fu)^2 + (v + fv)^2 <= 0.01 * (((u^2 + v^2) + fu^2) + fv^2) + 0.5
 *               (every pixel is consistent when flow_f is NULL)
 *   boundary    ux = (u(x+1, y) - u(x-1, y)) / 2 and uy, vx, vy likewise on the scaled flow, indices
 *               clamped to the picture (replicated border):
 *               ((ux^2 + uy^2) + vx^2) + vy^2 > 0.01 * (u^2 + v^2) + 0.002, or an unknown neighbour
 *   c           = known and inside and consistent and not boundary
 * The constants are Ruder's and are in pixels of the H x W at hand, whatever scale of a pyramid that
 * is: a flow scaled down to a coarse level meets the same absolute 0.5 and 0.002, so the tests are
 * relatively looser there.
 * Composite (Ruder's long-term rule with binary weights; called closest frame first, the closest
 * reliable frame wins):  first != 0 means the accumulators count as zero (there is no memset pass);
 * if the weight before is 0 and c holds, target = (float)value on the three planes and weight = 1;
 * else, if first, target = 0 and weight = 0; else both stay as they are.  Each pixel writes only its
 * own outputs; no atomics: the same inputs give the same bits.  Traffic with flow_f and first: flow_b
 * 8 + flow_f 8 + prev 12 read (the stencil's neighbours and the taps are other lanes' lines), target
 * 12 + weight 4 written: 44 B per pixel.  A null pointer other than flow_f, H < 2, W < 2 or a scale
 * factor that is not finite is STX_ERR_ARG.  Asynchronous.
 *
 * stx_image_temporal is the term, per element in float32:
 *   w' = min(max(weight, 0), 1), NaN as 0 (fractional weights are allowed)
 *   d  = (img - target) / 127.5f
 *   grad = (scale * w') * d + grad            loss = scale * 63.75 * sum w' * d^2
 * so grad is the exact derivative of loss, and at w' = 1 it is the auxiliary-image term's gradient
 * (stx_image_regularizers) at aux_scale = scale.  One pass; the sum goes through per-block partials
 * that are added in double in a fixed order.  grad is read and written at most once: a pixel with w' =
 * 0 is skipped and an element whose addend is zero is not written, so img == target wherever w' > 0,
 * or a weight of all zeros, gives a loss of exactly 0 and leaves every bit of grad alone.  The term
 * ignores the iteration's shift, like stx_image_lap.  A null pointer or H, W <= 0 is STX_ERR_ARG.
 * *loss_out (host) is written at the next stx_sync; asynchronous like stx_image_lap. */
int stx_image_flow_warp(stx_engine *e, const float *prev, const float *flow_b, const float *flow_f,
                        int H, int W, double su, double sv, int first, float *target, float *weight);
int stx_image_temporal(stx_engine *e, const float *img, float *grad, const float *target,
                       const float *weight, int H, int W, double scale, double *loss_out);

/* Optical flow for the term above, estimated from two grey frames: the robust variational method of
 * Brox, Bruhn, Papenberg, Weickert ("High Accuracy Optical Flow Estimation Based on a Theory for
 * Warping", ECCV 2004) in the discretisation of Sanchez, Monzon, Salgado ("Robust Optical Flow
 * Estimation", IPOL 2013): coarse to fine with warping, a lagged nonlinearity, red-black SOR.  Every
 * count is fixed; there is no stopping test.
 *
 * I1 (the frame the flow starts from) and I2 (the frame it points into) are [H][W] STX_DEVICE float32
 * in 0 ... 255; flow_out is [2][H][W] STX_DEVICE float32, plane 0 horizontal and plane 1 vertical: the
 * displacement w with I1(p) ~ I2(p + w(p)), which stx_image_flow_warp reads as flow_b when I1 is the
 * current frame.  No unknown markers are written.  Every value in between is float64 on the device,
 * each operation rounded once in the order written here (sums from left to right as bracketed).
 *   sample(P, qx, qy) on a picture P [H][W]: qx = min(max(qx, 0), W - 1), x0 = min(floor(qx), W - 2),
 *       fx = qx - x0 (y likewise; the taps of stx_image_flow_warp);  top = (1 - fx) * P[y0][x0] + fx *
 *       P[y0][x0+1], bottom the same on row y0 + 1, value = (1 - fy) * top + fy * bottom  (exact at
 *       whole coordinates, the last row and column included)
 *   resample(P, h, w): sample(P, (x + 0.5) * (W / w) - 0.5, (y + 0.5) * (H / h) - 0.5) for x < w, y < h
 *   dx(P) = (P[y][min(x+1, W-1)] - P[y][max(x-1, 0)]) / 2,  dy(P) likewise along y
 * Pyramid: level 0 is the input; h' = floor(h * eta + 0.5), w' likewise; a level is added while
 *   min(h', w') >= 16, up to `levels` of them.  sigma = 0.6 * sqrt(1 / (eta * eta) - 1), r =
 *   ceil(3 * sigma), k[i] = exp(-(i * i) / (2 * sigma * sigma)) for i = -r .. r, divided by their sum
 *   (added from -r up).  A level is resample(G, h', w') of the level below it, G its Gaussian: along x
 *   first, then along y, indices clamped, each a sum from i = -r up that starts at 0.
 * The coarsest level starts from u = v = 0; a finer one from u = resample(u_coarse, h, w) * (w /
 *   w_coarse), v = resample(v_coarse, h, w) * (h / h_coarse).
 * Per level, with A = I1's and B = I2's picture: Ax = dx(A), Ay = dy(A), Bx = dx(B), By = dy(B), Bxx =
 *   dx(Bx), Bxy = dy(Bx), Byy = dy(By).  Then `outer` times:
 *     Iz = sample(B, x + u, y + v) - A;  Ix, Iy, Ixx, Ixy, Iyy = sample of Bx, By, Bxx, Bxy, Byy there;
 *     Ixz = Ix - Ax, Iyz = Iy - Ay;  du = dv = 0
 *     `inner` times, with Su = u + du, Sv = v + dv:
 *       b  = (Iz + Ix * du) + Iy * dv;  gx = (Ixz + Ixx * du) + Ixy * dv;  gy = (Iyz + Ixy * du) + Iyy * dv
 *       psiD = 0.5 / sqrt((b * b + gamma * (gx * gx + gy * gy)) + eps * eps)
 *       psiS = 0.5 / sqrt((((dx(Su)^2 + dy(Su)^2) + dx(Sv)^2) + dy(Sv)^2) + eps * eps)
 *       g_n  = (alpha * (psiS(p) + psiS(n))) / 2 for the neighbours n = left, right, up, down, and 0 for
 *              one outside the picture;  gs = ((g_left + g_right) + g_up) + g_down
 *       A11 = psiD * (Ix * Ix + gamma * (Ixx * Ixx + Ixy * Ixy))
 *       A12 = psiD * (Ix * Iy + gamma * (Ixx * Ixy + Ixy * Iyy))
 *       A22 = psiD * (Iy * Iy + gamma * (Ixy * Ixy + Iyy * Iyy))
 *       c1  = psiD * (Ix * Iz + gamma * (Ixx * Ixz + Ixy * Iyz))
 *       c2  = psiD * (Iy * Iz + gamma * (Ixy * Ixz + Iyy * Iyz))
 *       `sor` sweeps, each two half-sweeps: the pixels with (x + y) even, then the odd ones.  A pixel of
 *       the half-sweep's colour takes, with s(S) = ((g_left * S_left + g_right * S_right) + g_up * S_up)
 *       + g_down * S_down (a neighbour outside: its index clamped, its weight 0):
 *         du = (1 - omega) * du + omega * ((((s(Su) - gs * u) - A12 * dv) - c1) / (A11 + gs))
 *         dv = (1 - omega) * dv + omega * ((((s(Sv) - gs * v) - A12 * du) - c2) / (A22 + gs))   (the new du)
 *         Su = u + du,  Sv = v + dv
 *     u = u + du, v = v + dv
 * flow_out = (float)u, (float)v of level 0.  Identical frames give a flow of exactly 0.  No atomics: the
 * same inputs give the same bits.  With levels = outer = inner = 1 and a small sor the call is one
 * linear solve.
 *
 * Asynchronous: the launches are queued on the engine's stream.  The workspace (about 300 bytes per pixel) is
 * the engine's; it is freed at the next stx_sync, when the call's work is done.  STX_ERR_ARG, before
 * anything is allocated or launched: a null pointer, H or W below 16 or above 32768, a parameter that is
 * not finite, alpha <= 0, gamma < 0, eta outside (0.25, 0.95), omega outside (0, 2), eps <= 0, or a
 * count below 1.  The defaults are alpha 18, gamma 6, eta 0.75, omega 1.8, eps 0.001, outer 5, inner 1,
 * sor 10 and as many levels as fit (any large count). */
typedef struct { double alpha, gamma, eta, omega, eps; int levels, outer, inner, sor; } stx_flow_params;
int stx_image_flow_estimate(stx_engine *e, const float *I1, const float *I2, int H, int W,
                            const stx_flow_params *p, float *flow_out);

/* Screened-Poisson output stage (Mechrez, Shechtman, Zelnik-Manor, "Photorealistic Style Transfer with
 * Screened Poisson Equation", BMVC 2017): the stylised picture keeps its colours and its gradients are pulled
 * to the content picture's.  Per channel the output f minimises
 *     sum_p (f_p - s_p)^2 + lambda * sum over edges pq ((f_p - f_q) - (c_p - c_q))^2
 * over the 4-connected grid, solved for the correction e = f - s from e = 0 by a fixed count of multigrid
 * W-cycles.  Every count is fixed; there is no stopping test.
 *
 * img (s) and content (c) are [3][H][W] STX_DEVICE float32 in one frame (BGR minus mean, as the iterate is kept);
 * out is [3][H][W] STX_DEVICE float32, distinct from both.  Every value in between is float64 on the device, each
 * operation rounded once in the order written here (sums from left to right as bracketed); a channel never reads
 * another.
 *   N(p): the neighbours left, right, up, down of p that lie inside the level; n(p) = |N(p)| as a double.
 *   S(a)_p = ((a_left + a_right) + a_up) + a_down, a neighbour outside the level entering as +0.0.
 *   d = (double)c - (double)s
 *   b = lambda * (n * d - S(d));  e = 0                                       (level 0)
 * Levels: level 0 is the picture; H' = ceil(H / 2), W' = ceil(W / 2), lambda' = lambda / 4.  A level is the
 *   coarsest when min(H, W) <= 2 or lambda <= 0.05 (at most 9 levels for lambda <= 1000).
 * Half-sweep of colour k on a level: every pixel with ((y + x) & 1) == k takes
 *     e = (b + lambda * S(e)) / (1 + lambda * n)
 *   (its neighbours are of the other colour).  A sweep "k first" is the half-sweeps k, then 1 - k.
 * Visit of level l (its e and b given):
 *   the coarsest level: 20 sweeps, 0 first.
 *   any other: 2 sweeps, 0 first;
 *     r = (b + lambda * S(e)) - (1 + lambda * n) * e  (never stored), and on level l + 1
 *     b'[Y][X] = (((r[2Y][2X] + r[2Y][2X+1]) + r[2Y+1][2X]) + r[2Y+1][2X+1]) / count, a child outside level l
 *     entering as +0.0 and count the existing children (1, 2 or 4);  e' = 0;
 *     two visits of level l + 1, the second continuing from the first's e';
 *     e = e + (0.75 * (0.75 * e'[Y][X] + 0.25 * e'[Y][Xn]) + 0.25 * (0.75 * e'[Yn][X] + 0.25 * e'[Yn][Xn]))
 *     with Y = y >> 1, Yn = Y + 1 for an odd y and Y - 1 for an even one, clamped to the level (X, Xn likewise);
 *     2 sweeps, 1 first.
 * `cycles` visits of level 0, then out = (float)((double)s + e).
 * Where s equals c bit for bit, b = +0 and e = +0 throughout, so out is s bit for bit.  No atomics and no
 * reductions: the same inputs give the same bits.  A cycle leaves 0.1 to 0.3 of the error for lambda up to 1000
 * (DESIGN.md 3.26); the host's default is 9 cycles.
 *
 * Asynchronous: the launches are queued on the engine's stream.  The workspace (e and b of every level, 64 bytes
 * per pixel) is the engine's; it is freed at the next stx_sync, when the call's work is done.  STX_ERR_ARG, before
 * anything is allocated or launched and with out untouched: a null pointer, H or W below 1 or above 32768, lambda
 * not finite, <= 0 or > 1000, cycles outside 1 .. 32, out overlapping img or content. */
int stx_image_poisson(stx_engine *e, const float *img, const float *content, float *out, int H, int W,
                      double lambda, int cycles);

/* ------------------------------------------------------------- single-kernel test hooks */
/* Direct entry points to the individual kernels, used by tests/ to check each against the
 * oracle (x, w, b, y: STX_DEVICE).  w is the Caffe layout [Cout][Cin][k][k]. */
int stx_op_conv_forward(stx_engine *e, const float *x, int Cin, int H, int W, const float *w,
                        const float *b, int Cout, int ksize, int relu, float *y);
int stx_op_conv_backward_data(stx_engine *e, const float *dy, int Cout, int H, int W,
                              const float *w, int Cin, int ksize, const float *relu_mask_data,
                              float *dx);
int stx_op_pool_forward(stx_engine *e, const float *x, int C, int H, int W, int mode, float *y);
int stx_op_pool_backward(stx_engine *e, const float *dy, const float *x, int C, int H, int W,
                         int mode, const float *relu_mask_data, float *dx);

/* The loss terms of one tapped blob, launched exactly as stx_sc_grad_tile launches them
 * (style_transfer.py:575-593), for direct comparison with num_utils.gram_matrix / ssymm / norm2 /
 * normalize (num_utils.py:53-71,85-87,143-147).  All arrays STX_DEVICE.
 * stx_op_style_terms:   G = tril(F F^T)/(C*h*w);  D = G - gram_target (lower triangle);
 *                       half_sumsq = 1/2 sum D^2;  s_out = sym(D) F;  abs_sum = sum |s_out|;
 *                       normalized_out = s_out / (abs_sum/n + EPS)      (either output may be NULL)
 * stx_op_content_terms: c = F - roll2(content, roll_xy)[:, oy:oy+h, ox:ox+w];
 *                       sums[0] = sum c^2, sums[1] = sum |c|;  normalized_out = c / (sums[1]/n + EPS)
 * Both synchronise before returning the host scalars. */
int stx_op_style_terms(stx_engine *e, const float *feat, int channels, int h, int w,
                       const float *gram_target, float *s_out, float *normalized_out,
                       double *half_sumsq, double *abs_sum);
/* stx_op_style_terms through a mask, the launches of a masked style target (stx_set_style_masks) on given
 * arrays: mask_map [mh][mw], the window at (oy, ox) of roll2(mask_map, roll_xy) in the map's own pixels.
 * out = {1/2 sum D^2, sum |m . S|, a}; sgrad_out = a m . (sym(D) Fm). */
int stx_op_masked_style_terms(stx_engine *e, const float *feat, int channels, int h, int w,
                              const float *mask_map, int mh, int mw, int oy, int ox, const int roll_xy[2],
                              const float *gram_target, float *sgrad_out, double out[3]);
/* The launches of a masked content target (stx_set_content_mask) on given arrays: content [channels][ch][cw]
 * and mask_map [ch][cw], the window at (oy, ox) of both rolled by roll_xy, in the maps' own pixels.
 * out = {1/2 sum m d^2, sum |m d|, a}; sgrad_out = a (m d). */
int stx_op_masked_content_terms(stx_engine *e, const float *feat, int channels, int h, int w,
                                const float *content, int ch, int cw, const float *mask_map, int oy, int ox,
                                const int roll_xy[2], float *sgrad_out, double out[3]);
/* The launches of a statistics target (stx_set_stat_targets) on given arrays (all STX_DEVICE; MU, SD [channels]):
 * out = {E / 2, sum |S|}; s_out = S. */
int stx_op_stat_terms(stx_engine *e, const float *feat, int channels, int h, int w, const float *MU,
                      const float *SD, float *s_out, double out[2]);
/* The launches of an NNFM target (stx_set_nnfm_targets) on given arrays (all STX_DEVICE; bank [rows][channels]):
 * out = {E, sum |S|}; s_out = S [channels][h][w]; index_out = j [h w].  An argument error leaves the outputs
 * alone: STX_ERR_ARG for a null pointer or rows <= 0, STX_ERR_UNSUPPORTED for channels % 64 != 0. */
int stx_op_nnfm_terms(stx_engine *e, const float *feat, int channels, int h, int w, const float *bank, int rows,
                      float *s_out, int *index_out, double out[2]);
/* ... and of a patch target (stx_set_nnfm_patch_targets): bank [rows][patch * patch * channels], 16-byte aligned.
 * patch 1 is stx_op_nnfm_terms; a patch other than 1 or 3 is STX_ERR_ARG.  Errors leave the outputs alone. */
int stx_op_nnfm_patch_terms(stx_engine *e, const float *feat, int channels, int h, int w, int patch,
                            const float *bank, int rows, float *s_out, int *index_out, double out[2]);
/* ... and of a k-nearest target (stx_set_nnfm_knn_targets): index_out = J [k][h w], rank-major, -1 from rank
 * min(k, rows) on.  k 1 is stx_op_nnfm_patch_terms; k outside 1 .. 4 is STX_ERR_ARG.  Errors leave the outputs
 * alone. */
int stx_op_nnfm_knn_terms(stx_engine *e, const float *feat, int channels, int h, int w, int patch, int k,
                          const float *bank, int rows, float *s_out, int *index_out, double out[2]);
/* ... and of a target with a coverage part (stx_set_nnfm_cover_targets): winner_out = i* [rows], out = {E, sum |S|,
 * E_cov}, E and S those of the sum.  cover 0 is stx_op_nnfm_knn_terms (out[2] and winner_out untouched); a cover
 * that is negative or not finite, or one other than 0 with patch 3, is STX_ERR_ARG.  Errors leave the outputs
 * alone. */
int stx_op_nnfm_cover_terms(stx_engine *e, const float *feat, int channels, int h, int w, int patch, int k, float cover,
                            const float *bank, int rows, float *s_out, int *index_out, int *winner_out, double out[3]);
/* ... and of a guided target (stx_set_nnfm_guided_targets; all arrays STX_DEVICE but seg_rows): bank [sum of
 * seg_rows][channels], mask_maps [segments][mh][mw], the window at (oy, ox) of each map rolled by roll_xy, in the
 * maps' own pixels.  s_out = S (without a); index_out = J [segments][k][h w], local to the segment, -1 in all k ranks
 * of the 128-column blocks in which no column has m_s > 0; out = {E, sum |S|, a}.  Errors leave the outputs alone. */
int stx_op_nnfm_guided_terms(stx_engine *e, const float *feat, int channels, int h, int w, int k, const float *bank,
                             const int *seg_rows, int segments, const float *mask_maps, int mh, int mw, int oy, int ox,
                             const int roll_xy[2], float *s_out, int *index_out, double out[3]);
/* The launches of a sliced Wasserstein target (stx_set_swd_targets) on given arrays (all STX_DEVICE; V
 * [dirs][channels], Tq [dirs][quantiles]): out = {E / 2, sum |S|}; s_out = S [channels][h][w]; rank_out (or null)
 * = r_d(i) [dirs][h w], which holds the sort to account.  Errors leave the outputs alone. */
int stx_op_swd_terms(stx_engine *e, const float *feat, int channels, int h, int w, const float *V, int dirs,
                     const float *Tq, int quantiles, float *s_out, int *rank_out, double out[2]);
/* The launches of a self-similarity target (stx_set_selfsim_targets) on two plain arrays [channels][h][w] (all
 * STX_DEVICE): the blob and, in place of the content map's window, an array of the blob's size.  sgrad = S
 * [channels][h][w], zero off the grid; sc = {E, sum |S|}; signs_out (or null) = T as int8 [N][N], which holds the
 * signs to account.  Errors leave the outputs alone. */
int stx_op_selfsim_terms(stx_engine *e, const float *feat, const float *content, int channels, int h, int w,
                         int points, float *sgrad, double sc[2], signed char *signs_out);
/* The launches of a shifted-Gram target (stx_set_shift_targets) on given arrays (feat, grams [n_offsets][channels]
 * [channels] and s_out STX_DEVICE; offsets host): out = {E / 2, sum |S|}; s_out = S [channels][h][w].  Errors leave
 * the outputs alone. */
int stx_op_shift_terms(stx_engine *e, const float *feat, int channels, int h, int w, const int *offsets,
                       int n_offsets, const float *grams, float *s_out, double out[2]);
/* The launches of a contextual target (stx_set_cx_targets) on given device arrays: feat [channels][h][w], bank
 * [rows][channels] and mu [channels] as stx_cx_bank gives them, sgrad [channels][h][w] = S; sc = {E, sum |S|}.
 * kbest_out (or null): k* as int32 [N]; winner_out (or null): i* as int32 [rows] -- the decisions to account.
 * Errors leave the outputs alone. */
int stx_op_cx_terms(stx_engine *e, const float *feat, int channels, int h, int w, int points, const float *bank,
                    const float *mu, int rows, double eta, float *sgrad, double sc[2], int *kbest_out,
                    int *winner_out);
int stx_op_content_terms(stx_engine *e, const float *feat, int channels, int h, int w,
                         const float *content, int content_h, int content_w, int oy, int ox,
                         const int roll_xy[2], float *normalized_out, double sums[2]);

/* Per-kernel-group timing for tuning and for bench.py's roofline figures: while enabled, every
 * launch group of the tile path (one conv / pool / Gram / SYMM / injection) is bracketed by HIP
 * events on the engine stream.  stx_profile_read synchronises, writes one line per group
 * "label<TAB>milliseconds<TAB>algorithmic_flops<TAB>MHz" into buf (NUL-terminated, truncated to
 * buf_len; *needed receives the full size) and clears the record.  MHz: the shader clock inside the
 * group's convolution kernel while stx_clock_marks is on (0 otherwise / for other groups). */
int stx_profile_enable(stx_engine *e, int on);
int stx_profile_read(stx_engine *e, char *buf, size_t buf_len, size_t *needed);

/* An audit of the maxima that the fp16-split kernels take over from earlier kernels (for the tests; off by
 * default, and then nothing is enqueued or allocated).  Those kernels -- the fp16-split convolution, Gram and
 * SYMM -- scale their operand by a power of two taken from 64 words of float bits that the kernel which wrote
 * the operand left behind, or that a pooling layer, a mask or a routed gradient passed on as a bound.  While
 * the audit is on, every such hand-off of a tile evaluation enqueues, in front of the consumer and on its
 * stream, a copy of the recorded words and a pass that measures max |x| over exactly the array the consumer
 * is about to read, both into storage of the audit's own: the slots the consumers read are not touched.
 * stx_amax_audit_read synchronises, writes one line per hand-off
 * "consumer<TAB>blob<TAB>data|diff<TAB>blob whose slots were read<TAB>recorded<TAB>measured" into buf (like
 * stx_profile_read; recorded = the largest slot, measured = the pass's result, both as float bits in
 * hexadecimal) and clears the record.  consumer: "fwd conv3_2", "bwd conv2_1", "style conv4_1", or "masked
 * style conv4_1" where the array is the masked feature map.  At most 2048 hand-offs are kept between two reads;
 * the evaluation that would exceed them fails. */
int stx_amax_audit(stx_engine *e, int on);
int stx_amax_audit_read(stx_engine *e, char *buf, size_t buf_len, size_t *needed);

/* Timing: ms spent by the GPU between the first and last kernel of the most recent FINISHED
 * stx_sc_grad_tile / stx_features_tile on this engine (HIP events on the engine stream; after
 * stx_sync that is the last call; while the host runs ahead it is the newest of the last four
 * that has completed, and only if none has does the call wait, for the newest). */
int stx_last_tile_ms(stx_engine *e, float *ms);

/* Matrix-core work of the convolutions of the same call: `algorithmic` counts every layer as a
 * direct convolution (2 * Cout * Cin * k * k * H * W, the figure SURVEY.md section 8d uses),
 * `issued` what the kernels actually put on the MFMA units (the Winograd kernels issue 2/3 or
 * 4/9 of it).  Gram / SYMM products are not included. */
int stx_last_tile_flops(stx_engine *e, double *algorithmic, double *issued);

/* The shader clock the GPU sustains INSIDE its dominant kernel (measurement only; nothing in the
 * reference corresponds).  While stx_clock_marks is on, one workgroup of every 2-D Winograd
 * convolution launch of this engine (the kernel that does 80 % of a tile evaluation's work) reads
 * the core-cycle counter and the constant 100 MHz counter before and after its chunk loop and
 * stores the two differences: the clock under exactly that load, with whatever the GPU's other
 * streams are running.  (Round 3 read the clock with a one-wave kernel BETWEEN the heavy kernels and
 * saw 2.43 GHz: the part clocks up the moment the matrix pipes go quiet; inside the convolutions it
 * sustains 2.0-2.3 GHz.)  stx_clock_marks_read synchronises the stream, returns the marks recorded
 * since the last read in MHz, launch order (*n_values <= max_values; at most 16384 are kept; 0
 * for a launch whose loop was shorter than a microsecond) and clears them.  bench.py switches them
 * on for its second, longer measurement only: the fp32 MFMA peak scales with this clock, which
 * depends on the kernels AND on their operands' bits.  With stx_profile_enable on as well,
 * stx_profile_read carries the mark of each convolution group as a fourth column. */
int stx_clock_marks(stx_engine *e, int on);
int stx_clock_marks_read(stx_engine *e, double *mhz, int max_values, int *n_values);

#ifdef __cplusplus
}
#endif
#endif /* STX_H_ */
