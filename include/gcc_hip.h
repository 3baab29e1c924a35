/*
 * gcc_hip.h -- C ABI of libgcc_hip.so: the MI355X (gfx950) kernels under the GCC training step.
 *
 * The reference (SJLeo/GCC) has no FFI layer: its hot path dispatches torch/ATen operators from
 * models/Pix2Pix.py.  Each entry point below names the reference call site(s) whose ATen operator
 * it replaces (paths relative to the reference root).  Conventions:
 *   - plain C, no torch types; every pointer is a DEVICE pointer owned by the caller (activations,
 *     weights, workspaces); the library allocates nothing.  What a launch does is decided by its arguments
 *     (the tile plan travels in gcc_conv_t.plan); the only process-wide state is the table of route switches below
 *     (gcc_set_option: atomics, defaults read once from GCC_* environment variables; the product leaves them alone), the one-time hipFuncSetAttribute of the kernels that use > 64 KB of LDS, and the RCCL entry
 *     points resolved on the first gcc_comm_* call (communicators themselves are explicit objects the caller owns);
 *   - every kernel is enqueued on the caller's `stream` and never synchronises;
 *   - return value: 0 = GCC_OK, negative = error (see gcc_strerror); no exceptions, no abort;
 *   - activations are NHWC bf16 (a PyTorch channels_last tensor): element (n,h,w,c) lives at
 *     ((n*H+h)*W+w)*ld + off + c, `ld` (pixel stride, elements) and `off` multiples of 8, and the
 *     bytes up to the next multiple of 8 channels are readable and zero;
 *   - conv weights are bf16 in two packings made by gcc_pack_weights from the fp32 master
 *     (a channels_last nn.Parameter, physical [Co][KH][KW][Ci]):  W  = [Co][KH*KW][Cip]  (fprop)
 *     and Wt = [Ci][KH*KW][Cop] (dgrad), Cip/Cop = channels rounded up to 8, zero filled;
 *   - fp32 everywhere else (statistics, losses, gradients of parameters, optimizer state).
 */
#ifndef GCC_HIP_H
#define GCC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gcc_stream_t; /* hipStream_t */

enum {
    GCC_OK = 0,
    GCC_ERR_BAD_ARG = -1,      /* null pointer / non-positive size / misaligned ld or offset */
    GCC_ERR_UNSUPPORTED = -2,  /* geometry outside what the kernels implement */
    GCC_ERR_WORKSPACE = -3,    /* workspace too small */
    GCC_ERR_LAUNCH = -4        /* hipGetLastError() after launch was not hipSuccess */
};

enum { GCC_ACT_NONE = 0, GCC_ACT_LRELU = 1, GCC_ACT_RELU = 2, GCC_ACT_TANH = 3 };

/* ABI generation of this header: bumped whenever a struct layout, an enum numbering or a prototype below changes.  gcc_version()
 * of the library a host loads must return exactly this number (gcc_amd/_lib.py refuses any other; an external host should check it
 * the same way): a stale .so reads gcc_conv_t.plan past its struct and sets the wrong option ids without any error. */
#define GCC_HIP_ABI 605

const char* gcc_strerror(int code);
int gcc_version(void); /* == GCC_HIP_ABI of the header the library was built from */
/* kernel launches the library has made in this process so far (reset != 0: return the count and start again from zero) */
long long gcc_launch_count(int reset);
/* Device-side error word.  The kernels that wait for other workgroups inside a launch (the grid InstanceNorm's tagged exchange,
 * gcc_inorm_fwd / gcc_inorm_bwd / gcc_bn_bwd_one_launch) bound every spin; a spin that expires stores a non-zero code into a
 * pinned host word, the launch's results are wrong, and every later call of those entry points returns GCC_ERR_LAUNCH.
 * Returns the word (0: no error; 0x1401: InstanceNorm exchange timed out; 0x1402: gcc_dw_inorm_fwd exchange timed out); clear
 * != 0 resets it.  Never synchronises. */
int gcc_device_error(int clear);

/* ---------------------------------------------------------------------------------------------
 * Route switches: which kernel family a geometry is routed to.  Every option only selects between kernels that compute the same
 * result: the tests set them to run a case down both routes and compare.  They are NOT the way a host chooses its schedule:
 * everything the model classes switch at run time (tile families, pair split, halo columns, weight-gradient split targets)
 * travels with the call in gcc_conv_t.plan, and the product runs with every option at its default (bench.py prints the vector
 * and refuses to run otherwise).  Defaults come from the environment variable of the same name (GCC_<NAME>) when it is set at
 * first use.  gcc_set_option(id, value): value < 0 restores the default; returns the previous value (>= 0) or GCC_ERR_BAD_ARG.
 * Process-wide atomics: set them while nothing is being launched.
 * The shipped library holds no diagnostic ablation: the "results are wrong" switches of the earlier rounds (main loops without
 * staging loads, a grid exchange made to time out) exist only in the GCC_DIAG_BUILD variant (csrc/build.sh: libgcc_hip_diag.so,
 * same ABI plus gcc_diag_set(bits)), which tests and probes load explicitly through GCC_HIP_LIB.
 * ------------------------------------------------------------------------------------------- */
enum {
    GCC_OPT_IGEMM_THIN = 0,     /* 1 (default): thin image-layer kernels; 2: without the LDS-staged wide (65..128 channel) data-gradient form; 0: none */
    GCC_OPT_FUSE_BN,            /* gcc_conv_bn_act: 3 (default; profiles/r4_summary.md): a split layer's K slices folded, statistics exchanged inside the
                                   launch and rows normalised by one kernel on the whole chip (bn_fold_grid_kernel; needs gcc_bn_t.tail_ws; other
                                   layers as 1); 2: BatchNorm finalized by the last-arriving workgroups of the launch that writes the statistic
                                   rows (gcc_bn_t.tail_ws), split layers folded by one full-chip kernel; 1: the round-2 form (a split layer's
                                   partials, statistics, finalize and normalise in one kernel of C / 8 workgroups); 0: separate launches */
    GCC_OPT_BN_BWD_SMALL,       /* 1 (default): gcc_bnact_bwd of <= 4096 pixels (training BatchNorm, no gate) runs as one kernel instead of
                                   three, gcc_channel_sum of <= GCC_CHANSUM_SMALL_MAX_PIXELS pixels as one instead of two */
    GCC_OPT_IGEMM_HALO,         /* 3 (default): also k3 s1 p1 convolutions on a 16-divisible grid (9 taps per staged slice: the VGG19 layers of SRGAN's
                                   perceptual loss, 10-25 % per layer, profiles/r4as_halo_3x3.txt); 2: also k4 s1 p1 convolutions on a 16-divisible grid (16 taps per staged slice); 1: k4 s2 p1 convolutions whose geometry fits (channels per tap a multiple of 64, 256 output channels
                                   per tile, output rows that tile 256 pixels) stage each 64-channel slice of the input neighbourhood of a
                                   256-pixel tile ONCE in LDS and serve the taps that share it from there (conv_halo.hip); 0: the gather
                                   kernel re-stages the pixels for every tap */
    GCC_OPT_INORM_GRID,         /* 1 (default): gcc_inorm_fwd / _bwd with a workspace split an image's plane over workgroups (in-launch barrier); 0: slab kernels */
    GCC_OPT_WGRAD_TS,           /* 1 (default): k4 s1 p1 weight gradients with channels in multiples of 64, >= 32 channel tiles and >= 16 pixel
                                   blocks per split, and k3 s1 p1 ones with channels in multiples of 64 and >= 128 workgroups of >= 8 blocks, run
                                   tap-stationary (wgrad_ts_kernel<4 / 3>: the 16 / 9 taps share one staged halo image of the input);
                                   2: wherever the geometry fits (tests); 0: wgrad_kernel only */
    GCC_OPT_HALO_XCD_COLS,      /* tile order of igemm_halo_kernel: 0: a pixel tile's column tiles are neighbours on one XCD (its L2 fetches the pixel
                                   slices once, every XCD streams all the weights); 1 (default): the stride-1 form gives every XCD one column tile
                                   (1 / ntiles of the weights per L2, pixel slices fetched by ntiles XCDs: the L4 forward fetches 108 MB instead of
                                   152 MB, same duration -- profiles/r4q_halo_xcd_cols.txt); 2: every form */
    GCC_OPT_COUNT_
};
int gcc_set_option(int id, int value);
int gcc_get_option(int id);
int gcc_options_default(void);      /* 1: every hook holds its built-in default */


/* ---------------------------------------------------------------------------------------------
 * Convolution geometry.  One descriptor serves Conv2d and ConvTranspose2d: a ConvTranspose2d
 * (models/Pix2Pix.py:40-56) is described by the Conv2d it is the adjoint of (big image = conv
 * input, small image = conv output) and run "backwards" (its forward = gcc_conv_dgrad, its
 * input-gradient = gcc_conv_fprop, its weight-gradient = gcc_conv_wgrad with x := grad of its
 * output and dy := its input).
 * ------------------------------------------------------------------------------------------- */
/* The tile plan of a convolution call travels WITH the call (round 5: it used to be process-wide option state, which two
 * models -- or two host threads -- with different schedules had to re-apply in turns).  Every field: 0 = the library's default.
 * The functions that size workspaces or statistic rows (gcc_conv_workspace, gcc_conv_stat_tiles, gcc_conv_bn_act_workspace,
 * gcc_conv_wgrad_workspace ...) read the plan of the descriptor they are given: pass them the descriptor the launch gets. */
typedef struct {
    int tile_families;  /* fprop / dgrad: 1: 128-pixel tiles only; 2: + 256x128; 3 (default): + 256x256 */
    int big_min;        /* minimum number of 256-pixel tiles of a launch (default 120: half a chip of one-per-CU workgroups; the rest of
                           the CUs run the other streams' kernels -- measured +2.7 % on the step against 200, profiles/r02_e) */
    int big_nk;         /* minimum K depth in 64-steps for 256-pixel tiles (default 24) */
    int pair;           /* 1: a 256x256-tile launch of < 192 tiles with >= 48 K steps runs two workgroups per tile (one per K half,
                           combined inside the launch through the caller's workspace) and fills the chip by itself: the plan for a
                           launch that has the chip to itself (single-stream schedules: 0.317 against 0.281 of the bf16 peak over the
                           step's igemm launches).  0 (default): one workgroup per tile -- less CU time per launch, the free CUs run
                           the other streams' kernels (the multi-stream production schedule: +1 % on the step) */
    int halo_hc;        /* columns per tile of igemm_halo_kernel: 0 (default): 256 where the layer tiles by 256 and such tiles are
                           enough to be routed (big_min), else 128; 1: also 128 where 256-column tiles would cover less than 3/4 of the
                           chip (PatchGAN L3 forward, L4 data gradient: 128 workgroups) -- the plan for a launch that has the chip to
                           itself, chosen together with `pair`; 128 / 256: forced (tests, A/B) */
    int wgrad_wgs_big;  /* workgroups a split 256x256 weight-gradient launch aims at (default 256) */
    int wgrad_wgs;      /* ... a split 128x128 weight-gradient launch (default 512) */
} gcc_conv_plan_t;

typedef struct {
    int N;            /* batch */
    int H, W;         /* conv INPUT spatial size */
    int Ci, Co;       /* logical channels */
    int KH, KW, stride, pad;
    int ldx, xoff;    /* conv-input tensor pixel stride / channel offset (elements) */
    int ldy, yoff;    /* conv-output tensor pixel stride / channel offset */
    gcc_conv_plan_t plan;   /* zero-filled: the library's defaults */
} gcc_conv_t;

static inline int gcc_conv_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

#define GCC_INORM_WORKSPACE_BYTES ((size_t)4096 + ((size_t)3 << 19))      /* gcc_inorm_fwd / _bwd, see there */
/* A BatchNorm2d (training statistics) that follows a convolution: nn.BatchNorm2d at models/Pix2Pix.py:34, 44-64, 286-298,
 * 320-341.  Handed to the conv (gcc_epilogue_t.bn, gcc_conv_bn_act) its coefficients are final when the call returns: where
 * the launch that writes the statistic rows can, its last-arriving workgroups fold them (no gcc_bn_finalize launch on the
 * chain; same bits as that launch: one canonical summation order) -- this needs `tail_ws`: GCC_TAIL_WORKSPACE_BYTES bytes,
 * zero-filled ONCE by the caller when it is allocated, used by ONE stream (its calls are ordered) and by nothing else; the
 * library leaves its counter words zero after every launch.  tail_ws NULL (or too small for the layer): a gcc_bn_finalize
 * launch inside the call instead. */
#define GCC_TAIL_WORKSPACE_BYTES ((size_t)4096 + ((size_t)4 << 20) + GCC_INORM_WORKSPACE_BYTES)   /* the last part: gcc_conv_bn_act's grid fold kernel */
typedef struct {
    const float* gamma; const float* beta;          /* [C] */
    float eps, momentum;
    double count;                                   /* N * H * W of the conv output */
    float* running_mean; float* running_var;        /* [C] or NULL */
    float* mean; float* rstd; float* scale; float* shift;   /* [C] outputs (saved for the backward pass) */
    void* tail_ws; size_t tail_ws_bytes;            /* see above; may be NULL / 0 */
    int finalize_in_launch;                         /* 1: the launch that writes the statistic rows may finalize (needs tail_ws); 0: always a
                                                       gcc_bn_finalize launch (tail_ws then only serves gcc_conv_bn_act's grid fold kernel) */
    int pad_;
} gcc_bn_t;

/* fused epilogue of fprop / dgrad: out = act(acc + bias[c]); optional per-tile BatchNorm partial
 * statistics (sum, sum of squares of the bf16-rounded outputs) for gcc_bn_finalize. */
typedef struct {
    const float* bias;    /* [channels] or NULL */
    int act;              /* GCC_ACT_* */
    float slope;          /* LeakyReLU slope */
    float* stats_partial; /* NULL, or [gcc_conv_stat_tiles()][2][channels] fp32 */
    void* workspace;      /* NULL, or gcc_conv_workspace() bytes: lets small-grid launches (U-Net bottleneck,
                             1-channel PatchGAN head) split their K loop over more workgroups */
    size_t workspace_bytes;
    const gcc_bn_t* bn;   /* NULL, or (with stats_partial) the BatchNorm behind this conv: finalized inside the call */
    /* NULL, or a second output written by the same launch: y2[.., y2off + c] = f(out) -- y2_mode 1: relu(out) (the in-place
     * LeakyReLU / ReLU pair the first U-Net skip is read through, models/Pix2Pix.py:33, 50, 77); 2: out * y2_gate[c] (the first
     * DifferentiableOP of the masked PatchGAN, models/Pix2Pix.py:320-322).  Served where gcc_conv_y2_supported() says 1 (the
     * thin image-layer forward route); GCC_ERR_UNSUPPORTED otherwise -- callers keep a gcc_bnact_fwd for that case. */
    void* y2; int ldy2, y2off, y2_mode; const float* y2_gate;
} gcc_epilogue_t;

/* scratch a fprop (dgrad=0) / dgrad (dgrad=1) launch can use: split-K partial tiles of small grids, or the hand-off slabs of a
 * pair-split 256x256-tile launch; 0 when the launch needs none.  Without it the launch simply runs un-split. */
size_t gcc_conv_workspace(const gcc_conv_t* c, int dgrad);

/* number of partial-statistics rows a fprop/dgrad call writes or zero-fills (one per pixel tile of the route the plan picks) */
int gcc_conv_stat_tiles(const gcc_conv_t* c, int dgrad);

/* kernel family a fprop / dgrad call runs on: 0 igemm_kernel, 1 the thin image-layer kernels (<= 8 channels on the
 * image side), 2 the single-output-channel head route, 3 the thin-output kernels for wide filters with <= 3 output channels
 * (conv_thinout.hip, round 5), 4 the ring-walk kernel for 3 x 3 stride-1 layers between <= 64-channel tensors (conv_ring3.hip,
 * round 5); < 0 for an invalid geometry.  Introspection for profilers. */
int gcc_conv_route(const gcc_conv_t* c, int dgrad, const gcc_epilogue_t* ep);
/* 1 when a call with this geometry / epilogue can write ep->y2 (see gcc_epilogue_t) */
int gcc_conv_y2_supported(const gcc_conv_t* c, int dgrad, const gcc_epilogue_t* ep);
/* tile the current plan picks for a geometry on the igemm_kernel route: BP * 1000 + BC (e.g. 256256 = 256 pixels x
 * 256 channels); 0 for an invalid geometry.  Introspection for tests and profilers. */
int gcc_conv_tile(const gcc_conv_t* c, int dgrad);
/* gcc_conv_route's 0 covers igemm_kernel and the LDS-resident-neighbourhood kernel of conv_halo.hip: 1 + the halo kernel's mode
 * (1: k4 s2 forward, 2: k4 s2 data gradient per phase, 3: the 128-channel data gradient with both px phases, 4 / 5: stride-1
 * forward / data gradient, k4 or k3) when a call with this geometry, plan and options runs on it; 0 when it runs on anything
 * else.  The call is taken to have a plain epilogue: bias / activation, and statistic rows when with_stats != 0 -- not
 * gcc_epilogue_t.bn without statistic rows and not gcc_epilogue_t.y2, which send a call to other routes and are not modelled
 * here.  Introspection for tests. */
int gcc_conv_halo_mode(const gcc_conv_t* c, int dgrad, int with_stats);

/* y = conv(x, W) (+bias, act).  Replaces aten::convolution at models/Pix2Pix.py:31-32, 280-300,
 * 320-343, 407-409 (F.conv2d / nn.Conv2d.forward).  x: [N,H,W,ldx]  w: W packing  y: [N,Ho,Wo,ldy] */
int gcc_conv_fprop(const gcc_conv_t* c, const void* x, const void* w, void* y,
                   const gcc_epilogue_t* ep, gcc_stream_t stream);

/* dx = conv_backward_data(dy, Wt) (+bias, act) -- also ConvTranspose2d.forward.  Replaces
 * aten::convolution_backward (grad_input) for the layers above and aten::convolution(transposed)
 * at models/Pix2Pix.py:40-56.  dy: [N,Ho,Wo,ldy]  wt: Wt packing  dx: [N,H,W,ldx] */
int gcc_conv_dgrad(const gcc_conv_t* c, const void* dy, const void* wt, void* dx,
                   const gcc_epilogue_t* ep, gcc_stream_t stream);

/* dW (+)= conv_backward_weight(x, dy) into the fp32 master layout [Co][KH*KW][Ci].  Replaces
 * aten::convolution_backward (grad_weight).  ws: workspace of gcc_conv_wgrad_workspace() bytes
 * (split-K slabs); accumulate != 0 adds into dw (PyTorch .grad accumulation semantics). */
size_t gcc_conv_wgrad_workspace(const gcc_conv_t* c);
int gcc_conv_wgrad(const gcc_conv_t* c, const void* x, const void* dy, float* dw, int accumulate,
                   void* ws, size_t ws_bytes, gcc_stream_t stream);

/* A GROUP of weight gradients as one launch (+ one fold launch): the backward pass of a generator yields a dozen small layers whose
 * weight gradients each fill a fraction of the chip (models/Pix2Pix.py:20-130: 14 regular ones per U-Net pass; aten runs one
 * convolution_backward per layer at :576 loss_G.backward()).  Entry i is what gcc_conv_wgrad(&c, x, dy, dw, accumulate, ..) would
 * compute; the pixel splits are planned for the group as a whole.  Only regular entries (Ci % 8 == 0, dw 16-byte aligned, no head /
 * thin-output geometry): gcc_conv_wgrad_group_workspace returns 0 for a group that holds any other, and the caller keeps such layers
 * on gcc_conv_wgrad.  Protocol (the library allocates nothing and copies nothing to the device):
 *   bytes = gcc_conv_wgrad_group_workspace(items, n)                      -- DEVICE workspace for the slabs (persistent: its address
 *                                                                            is part of the table)
 *   gcc_conv_wgrad_group_prepare(items, n, ws, bytes, table_host)         -- fills gcc_conv_wgrad_group_table_bytes() bytes of HOST
 *                                                                            memory; the caller copies them to device memory ONCE
 *   gcc_conv_wgrad_group_run(table_dev, table_host, stream)               -- every iteration: two launches
 * A table stays valid while the pointers and geometries it was prepared from do.  Fixed summation order: same bits run after run. */
#define GCC_WGRAD_GROUP_MAX 32
typedef struct {
    gcc_conv_t c;
    const void* x;
    const void* dy;
    float* dw;
    int accumulate;
} gcc_wgrad_item_t;
size_t gcc_conv_wgrad_group_table_bytes(void);
size_t gcc_conv_wgrad_group_workspace(const gcc_wgrad_item_t* items, int n);
int gcc_conv_wgrad_group_prepare(const gcc_wgrad_item_t* items, int n, void* ws, size_t ws_bytes, void* table_host);
int gcc_conv_wgrad_group_run(const void* table_dev, const void* table_host, gcc_stream_t stream);

/* weight gradient when channel dimensions are concatenations (see gcc_pack_desc_t): `c` describes the
 * PHYSICAL problem (c->Co = padded rows, c->Ci = padded cols); dw is the logical master-layout gradient
 * [rows][taps][cols]. */
int gcc_conv_wgrad_seg(const gcc_conv_t* c, const void* x, const void* dy, float* dw, int rows, int cols,
                       int row_split, int col_split, int accumulate, void* ws, size_t ws_bytes, gcc_stream_t stream);

/* fp32 master [rows][taps][cols] -> bf16 W [rows][taps][ceil8(cols)] and Wt [cols][taps][ceil8(rows)].
 * Either output may be NULL. */
int gcc_pack_weights(const float* master, int rows, int taps, int cols, void* w, void* wt,
                     gcc_stream_t stream);

/* multi-tensor form: DEVICE arrays built once per optimizer group.  kind 0: W chunk `a` (2048 output
 * elements); kind 1: one 32x32 tile (row block b, column block c) of tap `a` for Wt; kind 2 (unsplit tensors with
 * cols % 4 == 0 and a 16-byte aligned master): W and Wt of one 64x64 tile of tap `a` from a single read of the master. */
/* rows / cols are the master's logical sizes; row_split / col_split (0 = none) say that the dimension is
 * a concatenation whose first part has that many channels: each part is padded to 8 channels in the
 * packings (W = [rowsp][taps][colsp], Wt = [colsp][taps][rowsp], rowsp/colsp = padded physical sizes),
 * matching activation buffers in which the two tensors sit in 8-aligned channel slices. */
typedef struct { const float* master; void* w; void* wt; int rows, taps, cols, colsp, rowsp, row_split, col_split, pad_; } gcc_pack_desc_t;
typedef struct { int tensor, kind, a, b, c, pad_; } gcc_pack_item_t;
int gcc_pack_weights_multi(const gcc_pack_desc_t* descs, const gcc_pack_item_t* items, int nitems,
                           gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Tensor packing between the public NCHW fp32 surface and NHWC bf16.
 * Replaces torch.cat((real_A, fake_B), 1) at models/Pix2Pix.py:467,471,494,499,516 and the
 * host->device staging of set_input (:456-457).
 * ------------------------------------------------------------------------------------------- */
/* dst[n,h,w,dstoff + c] = bf16(src[n,c,h,w]) for c < C ; channels [C, Cfill) zero-filled. */
int gcc_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int N, int C, int H, int W, int ld, int off,
                              int Cfill, gcc_stream_t stream);
int gcc_nhwc_bf16_to_nchw_f32(const void* src, float* dst, int N, int C, int H, int W, int ld, int off,
                              gcc_stream_t stream);
/* channel-slice copy between NHWC bf16 tensors: dst[.., doff+c] = src[.., soff+c], c < C (C%8==0 not
 * required; [C, Cfill) zero-filled in dst). */
int gcc_nhwc_copy(const void* src, int lds, int soff, void* dst, int ldd, int doff, int C, int Cfill,
                  size_t pixels, gcc_stream_t stream);
/* The kernel gcc_nhwc_copy (and gcc_nhwc_add, with Cfill = C) runs a window on: 0 vector (16-byte accesses: lds, soff, ldd, doff
 * and C multiples of 8, nothing to zero-fill), 1 group (source and destination window each inside one aligned 8-channel group of
 * rows that are multiples of 8: one 16-byte read-modify-write per pixel), 2 scalar; GCC_ERR_BAD_ARG for a window the entries
 * refuse (C <= 0, a negative offset, soff + C > lds, doff + max(C, Cfill) > ldd).  Host only: the entries decide by this call. */
int gcc_nhwc_copy_route(int lds, int soff, int ldd, int doff, int C, int Cfill);
/* channel concatenation of two thin tensors into one 8-wide group: dst[.., doff + c] = a[.., aoff + c] (c < Ca), then
 * b[.., boff + c] (c < Cb), zeros up to 8 (Ca + Cb <= 8).  Replaces torch.cat((real_A, fake_B), 1) at
 * models/Pix2Pix.py:466-470, 483 (the discriminator's conditional input). */
int gcc_nhwc_pack_pair(const void* a, int lda, int aoff, const void* b, int ldb, int boff, void* dst, int ldd, int doff,
                       int Ca, int Cb, size_t pixels, gcc_stream_t stream);
/* dst[.., doff+c] += src[.., soff+c]  (gradient fan-in of fake_B: models/Pix2Pix.py:516-550) */
int gcc_nhwc_add(const void* src, int lds, int soff, void* dst, int ldd, int doff, int C, size_t pixels,
                 gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d (training / eval) fused with activation, DifferentiableOP gate and dropout.
 * Replaces aten::native_batch_norm(+_backward), leaky_relu_, relu_, bernoulli_/mul (Dropout) and
 * the mask multiply of models/DifferentiableOp.py:44-49 at models/Pix2Pix.py:33-36, 57-64, 286-298,
 * 320-341.
 * ------------------------------------------------------------------------------------------- */
/* Reduce the per-tile partial sums over `count` pixels into batch statistics; writes
 * mean/rstd (saved for backward), scale = gamma*rstd, shift = beta - mean*scale and updates
 * running_mean/var (momentum, unbiased variance) when they are non-NULL. */
int gcc_bn_finalize(const float* stats_partial, int tiles, int C, double count, const float* gamma,
                    const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                    float* mean, float* rstd, float* scale, float* shift, gcc_stream_t stream);
/* InstanceNorm2d(affine=False, no running statistics; models/Pix2Pix.py:201, models/CycleGAN.py:145): per image
 * and channel mean / rstd from [groups][tiles_per_group][2][C] partial sums (conv epilogue or gcc_channel_stats) */
int gcc_in_finalize(const float* stats_partial, int tiles_per_group, int groups, int C, double count, float eps,
                    float* mean, float* rstd, float* scale, float* shift, gcc_stream_t stream);
/* The same InstanceNorm (+ activation, + residual added after it) in one launch: statistics, mean / rstd / scale / shift [N][C]
 * written for the backward, y = act((x - mean) rstd) + residual (models/CycleGAN.py:77-138 at batch 1).  With a workspace the
 * plane of an image is split over up to 256 / N workgroups (pixel ranges x 64-channel groups) that meet at an in-launch barrier; without one (NULL) a workgroup
 * owns a whole (image, 16-channel slab).  Workspace contract: GCC_INORM_WORKSPACE_BYTES bytes, zero-filled once by the
 * caller when it is allocated, used by ONE stream (calls on it are ordered) and by nothing else. */
int gcc_inorm_fwd(const void* x, int ldx, void* y, int ldy, const void* residual, int ld_residual, int C, int HW, int N,
                  int act, float slope, float eps, float* mean, float* rstd, float* scale, float* shift,
                  void* workspace, size_t workspace_bytes, gcc_stream_t stream);
/* Depthwise 3x3 convolution behind a ReflectionPad2d(1) and the InstanceNorm2d(affine=False) after it in ONE launch: the
 * MobileResnet blocks' eval-mode forward (models/Pix2Pix.py:132-197, models/CycleGAN.py:77-138; MobileResnetEngine.infer).
 * Added without a GCC_HIP_ABI bump (additions only, no existing layout or numbering changed): a host built against this
 * header that loads an older library fails when it binds gcc_dw_inorm_fwd, not at the gcc_version() check.
 * Per image n and channel c < C, NHWC bf16, statistics over the H x W plane (biased variance, no affine):
 *   u = x                                   (GCC_DWIN_PLAIN: x is the block input)
 *   u = relu((p - mu_p) rho_p)              (GCC_DWIN_NORM_RELU: x = p, the raw output of the 1x1 conv in front)
 *   u = r + (p - mu_p) rho_p                (GCC_DWIN_RESIDUAL: x = p, r = the previous block's input; u is stored to u_out)
 *   d = dw3x3(ReflectionPad2d(1)(u)),  y = (d - mu_d) rho_d,  rho = 1 / sqrt(var + eps)
 * u is rounded to bf16 once (as the training route stores it) and the conv reads that value; d is never stored; y is rounded
 * once.  `bias` is not read: it cancels under the InstanceNorm (may be NULL).  Channels C .. ceil8(C) - 1 of y and u_out are
 * written as zeros.  Statistics: fp32 partials folded in double in one fixed order (the same bits on every run).  The
 * workgroups of an image meet at one (PLAIN) or two in-launch exchanges of the grid InstanceNorm (gcc_inorm_fwd); every spin
 * is bounded, an expired one stores 0x1402 into the device error word (gcc_device_error) and later calls return
 * GCC_ERR_LAUNCH.  Workspace contract as gcc_inorm_fwd's (zero-filled once, used by ONE stream), GCC_DW_INORM_WORKSPACE_BYTES
 * serves every geometry the plan takes.  GCC_ERR_BAD_ARG: unknown mode, a missing pointer the mode needs, an ld that is not a
 * multiple of 8 or below ceil8(C); GCC_ERR_UNSUPPORTED (nothing launched): the geometry is outside the grid plan (N > 64,
 * C > 2048, H or W < 2, more (image, 16-channel group) domains than the grid budget, planes wider than an LDS tile's rows,
 * about 500 pixels, more than 8 pixels per lane and sweep, where it no longer beats the launches it replaces);
 * GCC_ERR_WORKSPACE: workspace too small.
 * gcc_dw_inorm_route answers without launching: 1 (one launch) or the error code gcc_dw_inorm_fwd would return. */
enum { GCC_DWIN_PLAIN = 0, GCC_DWIN_NORM_RELU = 1, GCC_DWIN_RESIDUAL = 2 };
#define GCC_DW_INORM_WORKSPACE_BYTES ((size_t)4096 + ((size_t)3 << 20))
typedef struct {
    int mode;                           /* GCC_DWIN_* */
    const void* x; int ldx;             /* PLAIN: the block input u; otherwise p, the raw output of the preceding 1x1 conv */
    const void* r; int ldr;             /* RESIDUAL only: the previous block's input */
    void* u_out; int ldu;               /* RESIDUAL only: u stored (the next block's residual) */
    const float* w; const float* bias;  /* fp32 masters of nn.Conv2d(C, C, 3, groups=C): [C][9], [C] (bias not read) */
    void* y; int ldy;
    int N, H, W, C; float eps;
    void* workspace; size_t workspace_bytes;
} gcc_dw_inorm_t;
int gcc_dw_inorm_fwd(const gcc_dw_inorm_t* d, gcc_stream_t stream);
int gcc_dw_inorm_route(const gcc_dw_inorm_t* d);   /* 1: one launch; < 0: the code gcc_dw_inorm_fwd returns (nothing launched) */
/* One number of the plan the launch would use, answered by the launcher's own preparation (nothing launched): workgroups per
 * (image, channel group) S, workgroups one workgroup folds S1, exchange groups G, pixels per workgroup `rows`, channel groups per
 * image CG, 16-byte chunks per group CHg, pixel lanes per workgroup PL, pixels per LDS tile of a sweep.  < 0: the code
 * gcc_dw_inorm_route returns where the launch is declined; GCC_ERR_BAD_ARG for an unknown `what`.  Introspection for tests.
 * Added without a GCC_HIP_ABI bump (an addition). */
enum { GCC_DWIN_PLAN_S = 0, GCC_DWIN_PLAN_S1 = 1, GCC_DWIN_PLAN_G = 2, GCC_DWIN_PLAN_ROWS = 3, GCC_DWIN_PLAN_CG = 4,
       GCC_DWIN_PLAN_CHG = 5, GCC_DWIN_PLAN_PL = 6, GCC_DWIN_PLAN_TILE = 7 };
int gcc_dw_inorm_plan(const gcc_dw_inorm_t* d, int what);
/* its backward: dx = rstd (dz - mean(dz) - xhat mean(dz xhat)) with dz = g act'(y) (y NULL: the activation output is
 * recomputed from x); dx may alias g. */
int gcc_inorm_bwd(const void* x, int ldx, const void* y, int ldy, const void* g, int ldg, void* dx, int lddx, int C, int HW,
                  int N, int act, float slope, const float* mean, const float* rstd, void* workspace, size_t workspace_bytes,
                  gcc_stream_t stream);
/* BatchNorm backward with training statistics and nothing else fused (no gate, dropout or second gradient) in ONE launch
 * -- the SRResNet / SAGAN-generator blocks (models/SRGAN.py:19-66, models/SAGAN.py:77-140): dx = gamma rstd (dz - mean(dz) -
 * xhat mean(dz xhat)), dz = g act'(y) (y NULL: no activation), dgamma += sum dz xhat, dbeta += sum dz (either may be NULL).
 * workspace: as for gcc_inorm_fwd (the same one may be shared on a stream).  GCC_ERR_UNSUPPORTED when the geometry does not
 * fit the grid form: call gcc_bnact_bwd instead. */
int gcc_bn_bwd_one_launch(const void* x, int ldx, const void* y, int ldy, const void* g, int ldg, void* dx, int lddx, int C,
                          size_t pixels, int act, float slope, const float* mean, const float* rstd, const float* gamma,
                          float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, gcc_stream_t stream);
/* ... with the pieces the U-Net's layers need (models/Pix2Pix.py:33-64): y NULL with an activation (its input is recomputed through
 * the forward's affine form `scale` / `shift` and the regenerated dropout mask), a second incoming gradient g2 through act2 (the
 * skip path: g act'(y) + g2 act2'(y)), Dropout(drop_p) with the (seed, pixel * C + channel) counter of gcc_bnact_fwd.  Any
 * tensor size; GCC_ERR_UNSUPPORTED as above. */
int gcc_bn_bwd_one_launch_ex(const void* x, int ldx, const void* y, int ldy, const void* g, int ldg, const void* g2, int ldg2,
                             void* dx, int lddx, int C, size_t pixels, int act, int act2, float slope, float drop_p,
                             unsigned long long seed, const float* mean, const float* rstd, const float* scale, const float* shift,
                             const float* gamma, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                             gcc_stream_t stream);
int gcc_channel_stats_tiles(size_t pixels_per_group, int C);
int gcc_channel_stats(const void* x, int ld, int off, int C, size_t pixels_per_group, int groups, float* stats,
                      gcc_stream_t stream);
/* eval mode: scale/shift from running statistics */
int gcc_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int C, float* scale, float* shift,
                       gcc_stream_t stream);
/* ... and, for a backward pass through the eval-mode layer (gcc_bnact_bwd with bn_eval), the statistics it normalised with:
 * mean = running_mean, rstd = 1 / sqrt(running_var + eps) (either may be NULL).  Added without a GCC_HIP_ABI bump (an addition). */
int gcc_bn_eval_state(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                      int C, float* mean, float* rstd, float* scale, float* shift, gcc_stream_t stream);

typedef struct {
    const float* scale;   /* [C] or NULL (identity) */
    const float* shift;   /* [C] or NULL */
    const float* gate;    /* [C] gate mask m (0, .5, 1) or NULL */
    int gate_after_act;   /* 0: act(gate(bn(x)))  (models/Pix2Pix.py:327-332) ; 1: gate(act(x)) (:320-322) */
    int act;              /* activation written to y */
    float slope;
    int act2;             /* activation written to y2 (if y2 != NULL): y2 = act2(gate(bn(x))) */
    float drop_p;         /* dropout probability (0 = off); applied after bn, before act (U-Net up path) */
    uint64_t seed;        /* counter-based RNG: keep = hash(seed, element index) >= p */
    int groups;           /* <= 1: BatchNorm.  G > 1: InstanceNorm over G images -- `pixels` is per image, scale/shift
                             are [G][C] (gcc_in_finalize), x/y/y2/residual hold the G images back to back */
    int ld_residual;
    const void* residual; /* optional NHWC bf16 tensor added to y after the activation (ResNet block) */
} gcc_bnact_t;

/* y[.., yoff+c] = act(...) ; optional second output y2 (e.g. the ReLU'd copy that lands in the
 * concat buffer).  x/y/y2 are NHWC bf16 with their own ld/off. */
int gcc_bnact_fwd(const gcc_bnact_t* p, const void* x, int ldx, int xoff, void* y, int ldy, int yoff,
                  void* y2, int ldy2, int y2off, int C, size_t pixels, gcc_stream_t stream);

/* Conv2d / ConvTranspose2d + BatchNorm2d(training statistics) + activation (+ dropout, + a second activated copy) as ONE call:
 * the U-Net layer `conv -> BatchNorm2d -> LeakyReLU/ReLU[/Dropout]` of models/Pix2Pix.py:31-36, 40-64 (conv = fprop for
 * dgrad == 0, backward-data / ConvTranspose forward for dgrad == 1, as gcc_conv_fprop / gcc_conv_dgrad; bias-free).
 *   y_raw (the conv's own output, kept for the backward pass), then batch statistics of its bf16-rounded values, mean / rstd /
 *   scale / shift and the running-statistics update as gcc_bn_finalize, then y = act(drop(bn(y_raw))) and, if y2 != NULL,
 *   y2 = act2(drop(bn(y_raw))) as gcc_bnact_fwd (`act`: its scale / shift / gate / residual / groups fields are ignored).
 * Layers whose grid is split over K (the U-Net's <= 16x16 layers: a handful of output rows, thousands of K) run two launches --
 * the fp32 partial tiles, then one kernel that folds them, takes the statistics (f64), finalises and normalises: a workgroup
 * per 8 output channels owns every row of them -- instead of five (partials, fold, channel statistics, finalize, normalise);
 * every other layer runs the ordinary three kernels inside this one call.  ws: gcc_conv_bn_act_workspace() bytes. */
size_t gcc_conv_bn_act_workspace(const gcc_conv_t* c, int dgrad);
int gcc_conv_bn_act(const gcc_conv_t* c, int dgrad, const void* x, const void* w, void* y_raw, const gcc_bn_t* bn,
                    const gcc_bnact_t* act, void* y, int ldy, int yoff, void* y2, int ldy2, int y2off, void* ws,
                    size_t ws_bytes, gcc_stream_t stream);
/* One number of the plan that call would run, answered by the launcher's own decision code (nothing launched; the call's
 * workspace is taken to be the gcc_conv_bn_act_workspace() bytes it demands; bn: the call's descriptor -- its tail_ws decides
 * between the routes).  ROUTE: 0 the conv with statistic rows (gcc_conv_fprop / _dgrad's kernels, finalize in the launch or
 * by gcc_bn_finalize) + gcc_bnact_fwd; 1 partial tiles + splitk_bn_act_kernel; 2 partial tiles + bn_fold_grid_kernel on the
 * whole chip.  KSPLIT: the K slices behind the 4 MB cap (1: un-split).  LAUNCHES: kernel launches of the call (route 0 on the
 * thin-output, ring-walk or halo conv routes: GCC_ERR_UNSUPPORTED, those plan their own).  Route 2 only (GCC_ERR_BAD_ARG on the
 * others): S, S1, G, ROWS, CG, CHG, PL as GCC_DWIN_PLAN_* with the rows of all phases as one plane, PPT the rows-per-lane
 * instantiation of the kernel (1, 2, 4).  < 0: the code the call itself is declined with; GCC_ERR_BAD_ARG for an unknown `what`.
 * Introspection for tests.  Added without a GCC_HIP_ABI bump (an addition). */
enum { GCC_CONVBN_PLAN_ROUTE = 0, GCC_CONVBN_PLAN_KSPLIT = 1, GCC_CONVBN_PLAN_LAUNCHES = 2, GCC_CONVBN_PLAN_S = 3,
       GCC_CONVBN_PLAN_S1 = 4, GCC_CONVBN_PLAN_G = 5, GCC_CONVBN_PLAN_ROWS = 6, GCC_CONVBN_PLAN_CG = 7, GCC_CONVBN_PLAN_CHG = 8,
       GCC_CONVBN_PLAN_PL = 9, GCC_CONVBN_PLAN_PPT = 10 };
int gcc_conv_bn_act_plan(const gcc_conv_t* c, int dgrad, const gcc_bn_t* bn, int what);

/* ---------------------------------------------------------------------------------------------
 * Inference (eval-mode) convolution: the layers of SRGAN's generator (models/SRGAN.py:19-199) with BatchNorm in eval mode, i.e.
 * a per-channel affine map, folded into the conv's epilogue:
 *     y[p][c] = act(scale[c] * acc[p][c] + shift[c])  (+ residual[p][c])
 * in fp32 registers with ONE bf16 rounding on store; no statistics.  act: GCC_EVAL_ACT_*; the PReLU slope is a DEVICE scalar
 * (nn.PReLU() is learned: no host read).  Served by the ring-walk route (3 x 3 stride-1 layers between <= 64-channel tensors
 * of >= 8192 pixels, conv_ring3.hip) and by igemm_kernel (128-pixel tiles, split-K through `workspace` for small grids with a
 * long K loop) for every other forward geometry; forward only.  An internal route that cannot serve the epilogue declines
 * it (GCC_ERR_UNSUPPORTED) before it launches anything: the epilogue is never applied in part.
 * ------------------------------------------------------------------------------------------- */
enum { GCC_EVAL_ACT_NONE = 0, GCC_EVAL_ACT_PRELU = 1, GCC_EVAL_ACT_TANH = 2,
       GCC_EVAL_ACT_RELU = 3, GCC_EVAL_ACT_LRELU = 4 /* gcc_conv_eval_ex only: gcc_conv_fprop_eval rejects them */ };
typedef struct {
    const float* scale;       /* [Co] or NULL (1) */
    const float* shift;       /* [Co] or NULL (0): conv bias and BatchNorm shift, folded (gcc_bn_eval_coeffs_group) */
    const float* slope;       /* DEVICE scalar, GCC_EVAL_ACT_PRELU only */
    const void* residual;     /* NULL, or NHWC bf16 [N, Ho, Wo, ld_residual] added after the activation (channels < Co only:
                                 the output's pad channels stay zero whatever the residual's hold) */
    int ld_residual, residual_off;    /* multiples of 8 */
    int act;                  /* GCC_EVAL_ACT_* */
    int pad_;
    void* workspace;          /* NULL, or gcc_conv_eval_workspace(c) bytes (16-byte aligned): split-K of small grids */
    size_t workspace_bytes;
} gcc_eval_epilogue_t;
int gcc_conv_fprop_eval(const gcc_conv_t* c, const void* x, const void* w, void* y, const gcc_eval_epilogue_t* ep,
                        gcc_stream_t stream);
/* scratch gcc_conv_fprop_eval can use for a geometry (its own tile plan: 128-pixel tiles): split-K partial tiles of a small grid
 * with a long K loop; 0 when the call never splits */
size_t gcc_conv_eval_workspace(const gcc_conv_t* c);
/* route gcc_conv_fprop_eval takes for a geometry given `workspace_bytes` of scratch: 4 the ring-walk kernel, 5 igemm_kernel
 * split over K, 0 igemm_kernel un-split; < 0 for an invalid geometry.  Introspection for tests and profilers. */
int gcc_conv_eval_route(const gcc_conv_t* c, size_t workspace_bytes);

/* Eval-mode coefficients of many BatchNorms (and plain conv biases) in ONE launch: item i writes
 *     scale[c] = gamma[c] / sqrt(running_var[c] + eps)          (1 when running_var is NULL)
 *     shift[c] = beta[c] + (bias[c] - running_mean[c]) * scale[c]   (bias[c] when running_var is NULL)
 * gamma / beta / bias NULL: 1 / 0 / 0.  `items` is a DEVICE array of n entries (built once while the pointers stay valid). */
typedef struct {
    const float* gamma; const float* beta; const float* running_mean; const float* running_var;
    const float* bias;
    float* scale; float* shift;
    int C; float eps;
} gcc_bn_eval_item_t;
int gcc_bn_eval_coeffs_group(const gcc_bn_eval_item_t* items, int n, gcc_stream_t stream);

/* Inference convolution, forward or transposed, with up to two activated outputs: the U-Net's layers with eval-mode BatchNorm
 * (models/Pix2Pix.py:40-118).  With z = scale[c] * acc[p][c] + shift[c] in fp32:
 *     y [p][c] = act (z)    at (c->ldy, c->yoff)   -- transposed: at (c->ldx, c->xoff)
 *     y2[p][c] = act2(z)    at (ldy2, y2off)       (y2 NULL: no second store)
 * each rounded to bf16 once; no statistics.  act / act2: GCC_EVAL_ACT_NONE, _RELU, _LRELU (host `slope`) or _TANH.
 * transposed = 0: Conv2d forward (x: c->ldx / xoff, weights W).  transposed = 1: ConvTranspose2d forward, i.e. what
 * gcc_conv_dgrad computes from the same arguments (x plays dy: c->ldy / yoff; y plays dx: c->ldx / xoff; weights Wt), over the
 * stride^2 output parity phases.  Served by igemm_kernel's 128-pixel tiles, split over K through `workspace` on small grids.
 * Channels >= Co of y and y2 (up to the next multiple of 8) are written as zeros.  GCC_ERR_BAD_ARG: misaligned ldy2 / y2off, an
 * unknown or PReLU act, y2 overlapping y's channels.  A geometry no route serves returns GCC_ERR_UNSUPPORTED before anything is
 * launched. */
typedef struct {
    const float* scale;       /* [Co] or NULL (1) */
    const float* shift;       /* [Co] or NULL (0): conv bias and BatchNorm shift, folded (gcc_bn_eval_coeffs_group) */
    void* y2;                 /* NULL, or NHWC bf16 with the output's geometry: the second activated copy */
    int ldy2, y2off;          /* multiples of 8 */
    int act, act2;            /* GCC_EVAL_ACT_NONE / _RELU / _LRELU / _TANH */
    float slope;              /* negative-side slope of GCC_EVAL_ACT_LRELU (both outputs) */
    int pad_;
    void* workspace;          /* NULL, or gcc_conv_eval_ex_workspace(c, transposed) bytes (16-byte aligned): split-K */
    size_t workspace_bytes;
} gcc_eval_ex_epilogue_t;
int gcc_conv_eval_ex(const gcc_conv_t* c, int transposed, const void* x, const void* w, void* y, const gcc_eval_ex_epilogue_t* ep,
                     gcc_stream_t stream);
/* split-K scratch gcc_conv_eval_ex can use for a geometry; 0 when the call never splits */
size_t gcc_conv_eval_ex_workspace(const gcc_conv_t* c, int transposed);
/* route of gcc_conv_eval_ex given `workspace_bytes`: 5 igemm_kernel split over K (two launches: partial tiles, then the fold
 * with the whole epilogue), 0 igemm_kernel un-split (one launch); < 0 for an invalid geometry */
int gcc_conv_eval_ex_route(const gcc_conv_t* c, int transposed, size_t workspace_bytes);

/* Inference convolution in fp32 on the f32-input matrix instructions (v_mfma_f32_32x32x2_f32; gcc_amd/csrc/conv_f32.hip): the
 * evaluator networks at the reference's own precision.  x, y and the residual are NHWC FP32, the weights fp32:
 *     y[p][c] = act(scale[c] * acc[p][c] + shift[c] + residual[p][c])      -- the residual is added BEFORE the activation, as in
 * a ResNet block (gcc_conv_fprop_eval adds it after).  acc is the sum over K = KH KW Ci products in ONE order, which depends on
 * nothing but K: one workgroup per output tile walks K in steps of 16 (inside a step k, k + 4, k + 1, k + 5, ... of each half of
 * 8), every product an fmaf onto the running sum; no split-K, no atomics, no workspace.  A pixel's result therefore does not
 * depend on its batch or on the tile (or tile shape) it fell into.  One launch.  Added without a GCC_HIP_ABI bump (additions only).
 * Geometry: KH == KW in {1, 3, 7}, stride 1 or 2, dilation 1, 2 or 4 (taps at ih = oh stride - pad + kh dilation),
 *   pad == dilation (KH / 2), Ci == 3 or a multiple of 8, Co a multiple of 8, any pixel count; GCC_ERR_UNSUPPORTED otherwise.
 *   The plan of gcc_conv_t is not read.
 * Layout: ldx / xoff / ldy / yoff / ld_residual / residual_off in floats, multiples of 4; pointers 16-byte aligned; a window
 *   must fit its ld (x: ceil4(Ci) channels -- with Ci == 3 the fourth channel is read and ignored); dilation < 1, an act other
 *   than GCC_EVAL_ACT_NONE / _RELU, a null pointer: GCC_ERR_BAD_ARG.  Only channels [yoff, yoff + Co) of y are written.
 * Weights: fp32 [Co][Kp], row co holding k = (kh KW + kw) Cip + ci with Cip = 4 for Ci == 3 and Ci otherwise, zero-filled at
 *   ci >= Ci and from KH KW Cip up to Kp = the next multiple of 16 (gcc_conv_eval_f32_kp).
 * gcc_conv_eval_f32_route: the tile the call would take (0: 128 pixels x 128 channels, 1: 64 x 64, 2: 128 x 32), or the error
 *   the call would return for the geometry; launches nothing. */
typedef struct {
    const float* scale;     /* [Co] or NULL (1): folded BatchNorm */
    const float* shift;     /* [Co] or NULL (0) */
    const float* residual;  /* NULL, or NHWC fp32 with the output's geometry, added BEFORE the activation */
    int ld_residual, residual_off;
    int act;                /* GCC_EVAL_ACT_NONE | GCC_EVAL_ACT_RELU */
    int dilation;           /* >= 1; taps at ih = oh*stride - pad + kh*dilation */
} gcc_eval_f32_epilogue_t;
int gcc_conv_eval_f32(const gcc_conv_t* c, const float* x, const float* w, float* y, const gcc_eval_f32_epilogue_t* ep,
                      gcc_stream_t stream);
int gcc_conv_eval_f32_route(const gcc_conv_t* c, int dilation);
int gcc_conv_eval_f32_kp(int Ci, int KH, int KW);
/* gcc_conv_eval_f32_ex: gcc_conv_eval_f32 with the kernel's two sides and the two paddings independent -- the same kernel, weight
 * packing (gcc_conv_eval_f32_kp), epilogue, tile shapes and order of K; what a pixel gets does not depend on its batch or tile.
 * The FID Inception network at the reference's own precision (gcc_amd/metric/inception_fid.py, precision 'fp32'): 5 x 5, (1, 7),
 * (7, 1), (1, 3), (3, 1) and padding-0 3 x 3 convolutions.  One launch.  Added without a GCC_HIP_ABI bump (additions only).
 * Geometry: KH and KW each in {1, 3, 5, 7}; 0 <= pad_h <= dilation (KH / 2) and 0 <= pad_w <= dilation (KW / 2), zeros on both
 *   sides of a direction (taps at ih = oh stride - pad_h + kh dilation, iw = ow stride - pad_w + kw dilation), so Ho = (H + 2 pad_h
 *   - dilation (KH - 1) - 1) / stride + 1 and Wo alike; stride 1 or 2; dilation 1, 2 or 4; Ci == 3 or a multiple of 8; Co a
 *   multiple of 8: GCC_ERR_UNSUPPORTED otherwise.  A negative padding, or a map smaller than the kernel's span: GCC_ERR_BAD_ARG.
 * c->pad MUST BE 0: the paddings of this call are its arguments, and a descriptor that carries one of its own was filled in for
 *   another call -- GCC_ERR_BAD_ARG, not a convolution with a padding the caller did not mean.  The plan of gcc_conv_t is not read.
 * Layout, weights, epilogue and the other refusals: gcc_conv_eval_f32's.  Every refusal happens before anything is launched.
 * gcc_conv_eval_f32_ex_route: the tile the call would take (0 / 1 / 2 as above) or its error for the geometry; launches nothing. */
int gcc_conv_eval_f32_ex(const gcc_conv_t* c, int pad_h, int pad_w, const float* x, const float* w, float* y,
                         const gcc_eval_f32_epilogue_t* ep, gcc_stream_t stream);
int gcc_conv_eval_f32_ex_route(const gcc_conv_t* c, int pad_h, int pad_w, int dilation);
/* gcc_conv_eval_f32_act: gcc_conv_eval_f32_ex's kernel with sides up to 9, PReLU and tanh, and an optional PixelShuffle(2) store --
 * the same weight packing (gcc_conv_eval_f32_kp), tile shapes, single order of K and pad_h / pad_w arguments.  SRResNet at the
 * reference's own precision (engine.SRResNetEngine.infer, precision 'fp32'; models/SRGAN.py:139-199).  One launch.  Added without
 * a GCC_HIP_ABI bump (additions only); the two entries above keep their behaviour and their bits.
 *     y = act(fmaf(acc, scale[c], shift[c]) + residual)         act: GCC_EVAL_ACT_NONE | _RELU | _PRELU | _TANH
 *   PReLU is v >= 0 ? v : slope v with `slope` ONE DEVICE scalar read by the kernel (a learned parameter: the host does not read
 *   it); a null slope with _PRELU, or any other act, is GCC_ERR_BAD_ARG.  tanh is the device library's tanhf.
 * Geometry: KH and KW each in {1, 3, 5, 7, 9}; everything else, c->pad == 0 included, as gcc_conv_eval_f32_ex.
 * shuffle: 0, or 2 for nn.PixelShuffle(2): output channel co of Co = 4 C goes to channel yoff + (co >> 2) of pixel
 *   (2 oh + ((co >> 1) & 1), 2 ow + (co & 1)) of an [N][2 Ho][2 Wo] image with pixel stride ldy.  ldy >= yoff + Co / 4
 *   (GCC_ERR_BAD_ARG otherwise); Co a multiple of 32, so that a 32-lane store group covers whole sub-pixels, and no residual
 *   (GCC_ERR_UNSUPPORTED).  Any other value of shuffle: GCC_ERR_BAD_ARG.  One scalar slope commutes with the shuffle, so conv +
 *   PixelShuffle + PReLU is this one launch.  Only channels [yoff, yoff + Co) -- shuffled: [yoff, yoff + Co / 4) -- are written.
 * Every refusal happens before anything is launched.  gcc_conv_eval_f32_act_route: the tile (0 / 1 / 2) or the geometry's error. */
typedef struct {
    const float* scale;     /* [Co] or NULL (1) */
    const float* shift;     /* [Co] or NULL (0) */
    const float* residual;  /* NULL, or NHWC fp32 with the output's geometry, added BEFORE the activation */
    int ld_residual, residual_off;
    int act;                /* GCC_EVAL_ACT_NONE | _RELU | _PRELU | _TANH */
    int shuffle;            /* 0, or 2: the store is nn.PixelShuffle(2) */
    const float* slope;     /* DEVICE scalar, GCC_EVAL_ACT_PRELU only */
    int dilation;           /* >= 1 */
    int pad_;
} gcc_eval_f32_act_epilogue_t;
int gcc_conv_eval_f32_act(const gcc_conv_t* c, int pad_h, int pad_w, const float* x, const float* w, float* y,
                          const gcc_eval_f32_act_epilogue_t* ep, gcc_stream_t stream);
int gcc_conv_eval_f32_act_route(const gcc_conv_t* c, int pad_h, int pad_w, int dilation, int shuffle);
/* gcc_conv_eval_f32_unet: the U-Net generator's layers at the reference's own precision (engine.UnetEngine.infer, precision
 * 'fp32'; models/Pix2Pix.py:40-118): Conv2d(k4, s2, p1) and ConvTranspose2d(k4, s2, p1) in fp32 with up to two activated outputs.
 * A gather and a store of its own on gcc_conv_eval_f32's tile: its tile shapes, matrix instruction and ONE order of K (walked in
 * steps of 16, every product an fmaf onto the running sum; no split-K, no atomics, no workspace): an output element does not
 * depend on its batch, its tile or the tile shape.  One launch.  Added without a GCC_HIP_ABI bump (additions only); the three
 * entries above keep their bits.  With z = fmaf(acc, scale[c], shift[c]):
 *     y [p][c] = act (z)   at (c->ldy, c->yoff)
 *     y2[p][c] = act2(z)   at (ldy2, y2off)          (y2 NULL: no second store, act2 not read)
 *   act / act2: GCC_EVAL_ACT_NONE | _RELU | _LRELU | _TANH.  _LRELU is z >= 0 ? z : slope z with the host `slope`, one rounded
 *   multiply; tanh is the device library's tanhf.  There is no residual.
 * The descriptor is the LAYER's in both directions (unlike gcc_conv_eval_ex, which reads a transposed call as a data gradient):
 *   c->H, c->W, c->Ci, c->ldx, c->xoff describe the input x; c->Co, c->ldy, c->yoff the output y.
 *   transposed = 0: y is [N][H / 2][W / 2] (H, W >= 2, odd sizes round down), taps at ih = 2 oh - 1 + kh.
 *   transposed = 1: y is [N][2 H][2 W] (H, W >= 1).  Each of the four output parity phases (oh & 1, ow & 1) is a 2 x 2-tap gather
 *     over x with K = 4 Ci, stored at pixel stride 2: an even oh takes kh = 1 from ih = oh / 2 and kh = 3 from ih = oh / 2 - 1, an
 *     odd oh takes kh = 0 from ih = (oh + 1) / 2 and kh = 2 from ih = (oh - 1) / 2; ow alike.  Nothing is zero-stuffed.
 * Geometry: KH == KW == 4, stride 2, dilation 1; Ci a multiple of 8 (forward also 3, read as 4 with the fourth channel ignored);
 *   Co a multiple of 8; any N: GCC_ERR_UNSUPPORTED otherwise.  c->pad other than 1 is GCC_ERR_BAD_ARG.  The plan is not read.
 * Layout: ldx / xoff / ldy / yoff / ldy2 / y2off in floats, multiples of 4; pointers 16-byte aligned; a window must fit its ld;
 *   y2's window must not share a float with y's; an unknown act (act2 with y2), a null pointer, transposed other than 0 / 1:
 *   GCC_ERR_BAD_ARG.  Only channels [yoff, yoff + Co) of y and [y2off, y2off + Co) of y2 are written.
 * Weights, transposed = 0: gcc_conv_eval_f32's packing, fp32 [Co][Kp] with k = (kh 4 + kw) Cip + ci from Conv2d's [Co][Ci][4][4].
 *   transposed = 1: fp32 [4][Co][Kp], phase 2 (oh & 1) + (ow & 1) first; row co of phase (ph, pw) holds k = (2 th + tw) Ci + ci with
 *   th, tw in {0, 1}, the element [ci][co][1 - ph + 2 th][1 - pw + 2 tw] of ConvTranspose2d's [Ci][Co][4][4] (tap (th, tw) reads
 *   x at (ih, iw) = ((oh >> 1) + ph - th, (ow >> 1) + pw - tw)).
 *   Kp = gcc_conv_eval_f32_unet_kp(Ci, transposed): 16 Cip or 4 Ci rounded up to 16, zero-filled beyond.
 * Every refusal happens before anything is launched.  gcc_conv_eval_f32_unet_route: the tile (0 / 1 / 2 as above, chosen by the
 *   rows of one launch slice: N (H / 2) (W / 2) forward, N H W per phase transposed) or the geometry's error; launches nothing. */
typedef struct {
    const float* scale;     /* [Co] or NULL (1): folded BatchNorm */
    const float* shift;     /* [Co] or NULL (0): BatchNorm shift or the conv's bias */
    float* y2;              /* NULL, or NHWC fp32 with the output's geometry: the second activated copy */
    int ldy2, y2off;
    int act, act2;          /* GCC_EVAL_ACT_NONE | _RELU | _LRELU | _TANH */
    float slope;            /* negative-side slope of GCC_EVAL_ACT_LRELU (both outputs) */
    int pad_;
} gcc_eval_f32_unet_epilogue_t;
int gcc_conv_eval_f32_unet(const gcc_conv_t* c, int transposed, const float* x, const float* w, float* y,
                           const gcc_eval_f32_unet_epilogue_t* ep, gcc_stream_t stream);
int gcc_conv_eval_f32_unet_route(const gcc_conv_t* c, int transposed);
int gcc_conv_eval_f32_unet_kp(int Ci, int transposed);
/* gcc_conv_eval_f32_resnet: the MobileResnet generator's reflection-padded and transposed convolutions at the reference's own
 * precision (engine.MobileResnetEngine.infer, precision 'fp32'; models/Pix2Pix.py:132-265, models/CycleGAN.py:77-138;
 * gcc_amd/csrc/resnet_f32.hip).  Two gathers and a store of its own on gcc_conv_eval_f32's tile: its tile shapes, matrix
 * instruction and ONE order of K (walked in steps of 16, every product an fmaf onto the running sum; no split-K, no atomics, no
 * workspace): an output element depends on neither its batch nor its tile.  One launch.  Added without a GCC_HIP_ABI bump
 * (additions only); the four entries above keep their bits.  The generator's other convolutions (k3 s2 p1, 1 x 1) run on
 * gcc_conv_eval_f32_act.
 *     y[p][c] = act(fmaf(acc, scale[c], shift[c]))      act: GCC_EVAL_ACT_NONE | _RELU | _TANH (the device library's tanhf)
 * The descriptor is the LAYER's: c->H, c->W, c->Ci, c->ldx, c->xoff describe the input x; c->Co, c->ldy, c->yoff the output y.
 * kind = GCC_F32_RESNET_REFLECT: Conv2d(k, stride 1, padding 0) behind ReflectionPad2d(k / 2), y is [N][H][W].  The padding is
 *   index arithmetic in the gather: a tap at ih = oh - k / 2 + kh < 0 reads row -ih, one at ih >= H reads row 2 (H - 1) - ih; iw
 *   alike.  No padded copy of the map exists.  KH == KW in {7, 3}, stride 1, Ci == 3 (read as 4 with the fourth channel ignored)
 *   or a multiple of 8: GCC_ERR_UNSUPPORTED otherwise.  c->pad other than 0 (the conv has none of its own), H or W <= k / 2:
 *   GCC_ERR_BAD_ARG.  Weights: gcc_conv_eval_f32's packing, fp32 [Co][Kp] with k = (kh KW + kw) Cip + ci.
 * kind = GCC_F32_RESNET_TRANSPOSED3: ConvTranspose2d(k3, s2, p1, output_padding 1), y is [N][2 H][2 W] (H, W >= 1).  Each of the
 *   four output parity phases (ph, pw) = (oh & 1, ow & 1) is a gather over x stored at pixel stride 2; nothing is zero-stuffed.
 *   An even oh takes kh = 1 from ih = oh / 2; an odd oh takes kh = 2 from ih = (oh - 1) / 2 and kh = 0 from ih = (oh + 1) / 2
 *   when that is < H; ow alike.  The phases have 1, 2, 2 and 4 taps and each walks only its own K = (1 + ph) (1 + pw) Ci, rounded
 *   up to 16.  KH == KW == 3, stride 2, Ci a multiple of 8: GCC_ERR_UNSUPPORTED otherwise; c->pad other than 1: GCC_ERR_BAD_ARG.
 *   Weights: fp32 [4][Co][Kp], phase 2 ph + pw first, Kp = 4 Ci rounded up to 16 for every phase; row co of phase (ph, pw) holds
 *   k = (th (1 + pw) + tw) Ci + ci for th <= ph, tw <= pw: the element [ci][co][ph ? 2 - 2 th : 1][pw ? 2 - 2 tw : 1] of
 *   ConvTranspose2d's [Ci][Co][3][3] (tap (th, tw) reads x at ((oh >> 1) + th, (ow >> 1) + tw)); zeros from the phase's K to Kp.
 * Both kinds: Co a multiple of 8 (GCC_ERR_UNSUPPORTED).  Layout: ldx / xoff / ldy / yoff in floats, multiples of 4; pointers
 *   16-byte aligned; a window must fit its ld; an unknown kind or act, a null pointer: GCC_ERR_BAD_ARG.  Only channels
 *   [yoff, yoff + Co) of y are written.  Every refusal happens before anything is launched.
 * gcc_conv_eval_f32_resnet_route: the tile (0 / 1 / 2 as above, chosen by N H W rows) or the geometry's error; launches nothing.
 * gcc_conv_eval_f32_resnet_kp(Ci, kind, k): Kp of the packing (k: 7 or 3 for REFLECT, 3 for TRANSPOSED3). */
enum { GCC_F32_RESNET_REFLECT = 0, GCC_F32_RESNET_TRANSPOSED3 = 1 };
typedef struct {
    const float* scale;     /* [Co] or NULL (1) */
    const float* shift;     /* [Co] or NULL (0): the conv's bias */
    int act;                /* GCC_EVAL_ACT_NONE | _RELU | _TANH */
    int pad_;
} gcc_eval_f32_resnet_epilogue_t;
int gcc_conv_eval_f32_resnet(const gcc_conv_t* c, int kind, const float* x, const float* w, float* y,
                             const gcc_eval_f32_resnet_epilogue_t* ep, gcc_stream_t stream);
int gcc_conv_eval_f32_resnet_route(const gcc_conv_t* c, int kind);
int gcc_conv_eval_f32_resnet_kp(int Ci, int kind, int k);
/* gcc_dwconv3x3_reflect_f32: depthwise 3 x 3 convolution behind ReflectionPad2d(1) with bias, NHWC fp32 (x, y: pointers to the
 * first channel of the window, ldx / ldy >= C in floats, multiples of 4, 16-byte aligned; C a multiple of 4; H, W >= 2).
 *     y[p][c] = fmaf chain: acc = bias[c]; acc = fmaf(x[mirror(oh - 1 + kh, ow - 1 + kw)][c], w[kh 3 + kw][c], acc), kh, kw ascending
 * w: fp32 [9][C] (tap-major), bias: fp32 [C], both packed by the host.  One thread's outputs are 4 channels of a pixel.
 * stats: NULL, or gcc_inorm_f32_workspace(N, C, H W) bytes that receive the InstanceNorm partials of y in gcc_inorm_stats_f32's
 *   format from this same launch (a workgroup owns whole chunks of one image's pixels), so that gcc_inorm_apply_f32 can follow
 *   at once.  One launch.  GCC_ERR_WORKSPACE: stats_bytes too small.  Every refusal happens before anything is launched. */
int gcc_dwconv3x3_reflect_f32(const float* x, int ldx, float* y, int ldy, const float* w, const float* bias, int N, int H, int W,
                              int C, void* stats, size_t stats_bytes, gcc_stream_t stream);
/* InstanceNorm2d(affine = False) on NHWC fp32 in two launches, with no launch waiting for a workgroup of its own grid.
 * gcc_inorm_stats_f32: a plane of H W pixels is cut into chunks of consecutive pixels whose size depends on H W alone (not on N or
 *   on the grid); per (image, chunk, channel) it writes the chunk's mean and M2 = sum (x - mean)^2 as doubles, [N][chunks][2][C],
 *   formed from sums about a pivot (the chunk's first pixel) -- never E[x^2] - E[x]^2 of the raw values.  The workspace is the
 *   caller's, gcc_inorm_f32_workspace(N, C, H W) bytes, 16-byte aligned; there is NO zero-fill contract: every partial the apply
 *   launch reads was written by the stats launch before it.
 * gcc_inorm_apply_f32: every workgroup folds the partials of its channels in chunk order, in double (mean = sum n_k mean_k / HW,
 *   M2 = sum M2_k + n_k (mean_k - mean)^2), forms rstd = 1 / sqrt(M2 / HW + eps) (biased variance) and writes
 *       y = act((x - mean) rstd) + residual        act: GCC_EVAL_ACT_NONE | _RELU; the residual (NULL: none) is added AFTER the
 *   activation, as gcc_inorm_fwd does.  The difference and the product are formed in double and rounded once.  y may be x.
 *   An all-zero channel (a pad channel) comes out as zeros.  There is no finalize launch between the two.
 * x, y, residual: pointers to the first channel of the window, ld >= C in floats, multiples of 4, 16-byte aligned; C a multiple of
 *   4 (GCC_ERR_UNSUPPORTED).  GCC_ERR_WORKSPACE: workspace_bytes too small.  Every refusal happens before anything is launched. */
size_t gcc_inorm_f32_workspace(int N, int C, long long HW);
int gcc_inorm_stats_f32(const float* x, int ldx, int N, int H, int W, int C, void* workspace, size_t workspace_bytes,
                        gcc_stream_t stream);
int gcc_inorm_apply_f32(const float* x, int ldx, float* y, int ldy, const float* residual, int ld_residual, int N, int H, int W,
                        int C, int act, float eps, const void* workspace, size_t workspace_bytes, gcc_stream_t stream);
/* dst[n][c][h][w] = src[p][off + c] for c < C: the NHWC fp32 image of gcc_conv_eval_f32_act as the NCHW fp32 buffer the metric
 * kernels read (gcc_psnr_y_sse, gcc_ssim_y_sum).  off + C <= ld.  One launch. */
int gcc_nhwc_f32_to_nchw_f32(const float* src, float* dst, int N, int C, int H, int W, int ld, int off, gcc_stream_t stream);
/* dst[p][off + c] = src[n][c][h][w] for c < C and 0 for C <= c < cfill: an NCHW fp32 image as the NHWC fp32 input of
 * gcc_conv_eval_f32 (ld, off, cfill multiples of 4; off + cfill <= ld; dst 16-byte aligned).  One launch. */
int gcc_nchw_f32_to_nhwc_f32(const float* src, float* dst, int N, int C, int H, int W, int ld, int off, int cfill,
                             gcc_stream_t stream);

/* Image bytes of the reference's util.tensor2im: out[p][k] = (uint8)(((x + 1) * 0.5) * 255) of channel k < 3 of pixel p of an
 * NHWC bf16 tensor (ld, off: multiples of 8), evaluated in fp32 in that order with no contraction, then truncated (values
 * outside [-1, 1] are clamped to 0 / 255).  out: DEVICE uint8 [pixels][3].
 * gcc_image_to_u8_f32: the same arithmetic (one kernel text) on an NHWC fp32 image, ld >= off + 3 in floats. */
int gcc_image_to_u8(const void* x, int ld, int off, size_t pixels, void* out, gcc_stream_t stream);
int gcc_image_to_u8_f32(const float* x, int ld, int off, size_t pixels, void* out, gcc_stream_t stream);

/* Backward of y = act(gate(bn(x))) [dropout] given up to two upstream gradients:
 *   g  = g1 * act'(y)  +  g2 * act2'(y)     (g2 from the skip/concat path, may be NULL)
 *   dz = g * m[c]  (gate)       dalpha[c] = sum g * z   (z = bn(x), STE, no mask factor)
 *   dgamma[c] = sum dz*xhat, dbeta[c] = sum dz, dx = scale*(dz - mean(dz) - xhat*mean(dz*xhat))
 * Two launches: reduce (writes dz into `dz` and per-block partials into ws) then apply (dx over dz).
 * bn == 0 : no normalisation (plain act backward: dx = g*m, no statistics). */
typedef struct {
    int bn;                  /* 1: through BatchNorm (training statistics) */
    int bn_eval;             /* 1: BN used running stats (dx = dz*scale); mean / rstd are then the running statistics
                                (gcc_bn_eval_state), dgamma / dbeta the sums over the unscaled dz */
    const float* mean;       /* saved mean [C] */
    const float* rstd;       /* saved rstd [C] */
    const float* gamma;      /* [C] */
    const float* beta;       /* [C] */
    const float* gate;       /* mask [C] or NULL */
    int gate_after_act;
    int act; float slope;    /* activation of y  (y is what act' is evaluated on, in-place semantics) */
    int act2;                /* activation of the second consumer (g2) */
    float drop_p; uint64_t seed;
    float* dgamma; float* dbeta; float* dalpha;  /* [C] fp32, accumulated into (+=) ; any may be NULL */
    int groups;              /* G > 1: InstanceNorm backward (mean/rstd [G][C], no parameter gradients); workspace is
                                G * gcc_bnact_bwd_workspace() */
    int flags;               /* bit 0: the workspace was zero-filled when it was allocated, is used by ONE stream and by nothing but
                                gcc_bnact_bwd calls -- the finalize step then runs inside the reduce launch (its last-arriving
                                workgroups fold the partial rows; the library leaves the head of the workspace zero): two launches
                                instead of three */
} gcc_bnact_bwd_t;

size_t gcc_bnact_bwd_workspace(int C, size_t pixels);
int gcc_bnact_bwd(const gcc_bnact_bwd_t* p, const void* x, int ldx, int xoff, const void* y, int ldy, int yoff,
                  const void* g1, int ldg1, int g1off, const void* g2, int ldg2, int g2off,
                  void* dx, int lddx, int dxoff, int C, size_t pixels, void* ws, size_t ws_bytes,
                  gcc_stream_t stream);

/* same, for a layer whose producer already applied `in_act` to x (conv epilogue): dx *= in_act'(x) */
int gcc_bnact_bwd_ex(const gcc_bnact_bwd_t* p, int in_act, float in_slope, const void* x, int ldx, int xoff,
                     const void* y, int ldy, int yoff, const void* g1, int ldg1, int g1off, const void* g2,
                     int ldg2, int g2off, void* dx, int lddx, int dxoff, int C, size_t pixels, void* ws,
                     size_t ws_bytes, gcc_stream_t stream);

/* ReflectionPad2d (explicit copy; backward = adjoint gather) and the depthwise 3x3 convolution with
 * ReflectionPad2d(1) of MobileResnetBlock / SeparableConv2d (models/Pix2Pix.py:132-197).
 * gcc_dwconv3x3_reflect mode 0: out = conv(x) + bias ; mode 1: out = d(x) from dy.  w: fp32 [C][9] master. */
int gcc_reflect_pad(const void* src, int lds, void* dst, int ldd, int N, int H, int W, int C, int pad, int backward,
                    gcc_stream_t stream);
int gcc_dwconv3x3_reflect(int mode, const void* x, int ldx, const void* dy, int lddy, void* out, int ldo, const float* w,
                          const float* bias, int N, int H, int W, int C, gcc_stream_t stream);
size_t gcc_dwconv3x3_wgrad_workspace(int N, int H, int W, int C);
int gcc_dwconv3x3_reflect_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, float* dbias, int N, int H,
                                int W, int C, void* ws, size_t ws_bytes, gcc_stream_t stream);

/* per-channel sum over pixels of an NHWC bf16 tensor (bias gradients): out[c] (+)= sum x[..,c] */
int gcc_channel_sum(const void* x, int ld, int off, int C, size_t pixels, float* out, int accumulate,
                    void* ws, size_t ws_bytes, gcc_stream_t stream);
size_t gcc_channel_sum_workspace(int C, size_t pixels);
/* several channel sums of <= GCC_CHANSUM_SMALL_MAX_PIXELS pixels each (the bias gradients of the layers of one grouped weight
 * gradient) as ONE launch; entry i is gcc_channel_sum(x, ld, off, C, pixels, out, accumulate, ..) bit for bit.
 * n <= GCC_CHANSUM_GROUP_MAX; GCC_ERR_UNSUPPORTED when an entry has more pixels (the caller keeps it on gcc_channel_sum). */
#define GCC_CHANSUM_GROUP_MAX 24
#define GCC_CHANSUM_SMALL_MAX_PIXELS 16384   /* also the limit of gcc_channel_sum's one-launch form (GCC_OPT_BN_BWD_SMALL) */
typedef struct {
    const void* x;
    int ld, off, C;
    size_t pixels;
    float* out;
    int accumulate;
} gcc_chansum_item_t;
int gcc_channel_sum_group(const gcc_chansum_item_t* items, int n, gcc_stream_t stream);

/* gate mask m = (sign(alpha - tau) + 1) / 2.  models/DifferentiableOp.py:25-26,58-59 */
int gcc_gate_mask(const float* alpha, float tau, float* mask, int C, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Losses (forward value + gradient in one pass; scalars are fp32 device words).
 * ------------------------------------------------------------------------------------------- */
/* GANLoss.__call__, models/GANLoss.py:38-59.  mode 0 hinge, 1 lsgan, 2 vanilla(BCE logits), 3 wgangp.
 * pred: NHWC bf16 [pixels][ld] channel `off` (PatchGAN map, 1 channel).  loss (+)= weight * L ;
 * dpred (may be NULL) = weight * dL/dpred written as bf16 with the same layout. */
int gcc_gan_loss(int mode, int target_is_real, int for_discriminator, const void* pred, int ld, int off,
                 size_t pixels, float weight, float* loss, int accumulate, void* dpred,
                 void* ws, size_t ws_bytes, gcc_stream_t stream);
/* same loss; `loss` receives the unweighted value, dpred (+)= grad_weight * (*grad_weight_dev) * dL/dpred.
 * grad_weight_dev (device scalar, may be NULL) carries data-dependent signs of the arch loss without
 * a host round trip (models/Pix2Pix.py:479-487). */
int gcc_gan_loss_ex(int mode, int target_is_real, int for_discriminator, const void* pred, int ld, int off,
                    size_t pixels, float* loss, void* dpred, float grad_weight, const float* grad_weight_dev,
                    int dpred_accumulate, gcc_stream_t stream);
/* arch-step scalars: loss = | |Lfr-Lf| - dT | + w (Lr+Lf) and its partial derivatives c_fr, c_f
 * (w = 1/2: models/Pix2Pix.py:505-509, models/CycleGAN.py:410-414; w = 1: models/SAGAN.py:388-389) */
int gcc_arch_coeffs(const float* Lfr, const float* Lf, const float* Lr, const float* dT, float real_fake_weight,
                    float* loss, float* c_fr, float* c_f, gcc_stream_t stream);
/* mean |a-b| * weight (nn.L1Loss, models/Pix2Pix.py:520) over C channels; da = weight*sign(a-b)/count */
int gcc_l1_loss(const void* a, int lda, int aoff, const void* b, int ldb, int boff, int C, size_t pixels,
                float weight, float* loss, int accumulate, void* da, int ldda, int daoff,
                void* ws, size_t ws_bytes, gcc_stream_t stream);
/* nn.MSELoss (models/SRGAN.py:447, 457): weight * mean((a-b)^2); da = weight * 2 (a-b) / count */
int gcc_mse_loss(const void* a, int lda, int aoff, const void* b, int ldb, int boff, int C, size_t pixels,
                 float weight, float* loss, int accumulate, void* da, int ldda, int daoff,
                 void* ws, size_t ws_bytes, gcc_stream_t stream);
size_t gcc_loss_workspace(size_t pixels, int C);

/* Feature distillation, models/Pix2Pix.py:537-548 + :733-740, for one feature pair:
 *   gram(f) = F F^T /(c h w) per image (F = [C][HW]);  Lg = sqrt(mse(gram(f), gram(t))) ;
 *   Lc = sqrt(mse(f, t)).   f,t: NHWC bf16 [N][HW][ld].
 * squared != 0: the CycleGAN form (models/CycleGAN.py:516-517), plain MSE terms without the square root.
 * gcc_distill_fwd writes the two scalars (unweighted) into out[0..1] and keeps what backward needs
 * in ws; gcc_distill_bwd writes df = wg*dLg/df + wc*dLc/df (bf16, same layout as f). */
size_t gcc_distill_workspace(int N, int C, int HW);
int gcc_distill_fwd(const void* f, int ldf, int foff, const void* t, int ldt, int toff, int N, int C, int HW,
                    int squared, float* out2, void* ws, size_t ws_bytes, gcc_stream_t stream);
int gcc_distill_bwd(const void* f, int ldf, int foff, const void* t, int ldt, int toff, int N, int C, int HW,
                    int squared, float wg, float wc, void* df, int lddf, int dfoff, void* ws, size_t ws_bytes,
                    gcc_stream_t stream);
/* What a gcc_distill_fwd / gcc_distill_bwd call of this size does, from the launchers' own decision code (the workspace
 * layout, the weight-gradient split plan and fold choice, the tile choice and batch-1 route predicates of the 1x1 product);
 * launches nothing.  plan[GCC_DISTILL_PLAN_N]:
 *   OFF_SCAL .. OFF_DFG  byte offsets in the workspace of scal (fp32 Lg, Lc), Gf, Gt (fp32 [N][C][C]), S (bf16 [N][C][C]) and
 *                        dfg (bf16 [N][HW][C]);  WS_BYTES = gcc_distill_workspace()
 *   GRAM_SPLITS, GRAM_KPER  pixel splits of a Gram product and 64-pixel k-steps per split;  GRAM_COL_TILES x GRAM_CO_TILES its
 *                        128 x 128 output tiles;  GRAM_FOLD 0: written directly, 1: wgrad_reduce_flat_kernel, 2: wgrad_reduce_vec_kernel
 *   BWD_ROUTE            gcc_conv_route's answer for the 1x1 product at N == 1, 0 (igemm_kernel, problems on grid.y) at N > 1;
 *   BWD_BP, BWD_BC, BWD_NTILES, BWD_MTILES  its tile plan (route 0)
 *   FWD_LAUNCHES, BWD_LAUNCHES  kernel launches of one call (gcc_launch_count)
 * GCC_ERR_BAD_ARG for the sizes the two entries refuse (and a NULL plan). */
enum { GCC_DISTILL_PLAN_OFF_SCAL = 0, GCC_DISTILL_PLAN_OFF_GF, GCC_DISTILL_PLAN_OFF_GT, GCC_DISTILL_PLAN_OFF_S,
       GCC_DISTILL_PLAN_OFF_DFG, GCC_DISTILL_PLAN_WS_BYTES, GCC_DISTILL_PLAN_GRAM_SPLITS, GCC_DISTILL_PLAN_GRAM_KPER,
       GCC_DISTILL_PLAN_GRAM_COL_TILES, GCC_DISTILL_PLAN_GRAM_CO_TILES, GCC_DISTILL_PLAN_GRAM_FOLD, GCC_DISTILL_PLAN_BWD_ROUTE,
       GCC_DISTILL_PLAN_BWD_BP, GCC_DISTILL_PLAN_BWD_BC, GCC_DISTILL_PLAN_BWD_NTILES, GCC_DISTILL_PLAN_BWD_MTILES,
       GCC_DISTILL_PLAN_FWD_LAUNCHES, GCC_DISTILL_PLAN_BWD_LAUNCHES, GCC_DISTILL_PLAN_N };
int gcc_distill_plan(int N, int C, int HW, long long* plan);

/* ---------------------------------------------------------------------------------------------
 * SAGAN (models/SAGAN.py).
 * Spectral normalisation, SpectralNorm._update_u_v (:25-38), on the fp32 master W_bar [R][C][k][k] (channels_last for
 * k > 1; the reference's w.view(R, -1) column order c*T + t is kept for v, T = k*k): one power iteration that
 * overwrites u [R] and v [C*T], t_out = W_bar v (kept by the caller for the gradient of u), sigma = u . t_out, and
 * W_eff = W_bar / sigma (fp32, same layout; feed it to gcc_pack_weights).  Runs on every forward, eval included.
 * gcc_spectral_grad folds G = dL/dW_eff into the master's gradient:
 *   dW_bar += G/sigma + s u v^T,  du += s t_fwd,  dv += s W_bar^T u,   s = -<G, W_bar>/sigma^2
 * with the LIVE u, v and the forward call's own sigma / t (what the reference's autograd evaluates, see
 * csrc/spectral.hip).  du / dv may be NULL (generator: u, v are never trained; discriminator: set_requires_grad
 * switches them on, :513). */
size_t gcc_spectral_workspace(int R, int C, int T);
int gcc_spectral_power_iteration(const float* w_bar, float* u, float* v, int R, int C, int T, float* t_out,
                                 float* sigma_out, float* w_eff, void* ws, size_t ws_bytes, gcc_stream_t stream);
/* the same power iteration with W_eff written straight into the two bf16 packings of gcc_pack_weights (w: [R][T][C padded to 8],
 * wt: [C][T][R padded to 8]) instead of an fp32 tensor: 4 launches instead of 7 for what a spectrally normalised convolution's
 * forward does before its convolution (SpectralNorm.forward, models/SAGAN.py:56-70); same bits as the separate calls */
int gcc_spectral_power_iteration_pack(const float* w_bar, float* u, float* v, int R, int C, int T, float* t_out,
                                      float* sigma_out, void* w, void* wt, void* ws, size_t ws_bytes, gcc_stream_t stream);
/* the power iterations + packings of several layers (every spectrally normalised convolution of one network's forward pass:
 * the iterations depend on the weights alone, not on the activations) as FOUR launches instead of four per layer; entry i is
 * gcc_spectral_power_iteration_pack(w_bar, u, v, R, C, T, t_out, sigma_out, w, wt, ..) bit for bit.  n <= GCC_SPECTRAL_GROUP_MAX;
 * ws: gcc_spectral_group_workspace(items, n) bytes (every layer its own scratch), 16-byte aligned. */
#define GCC_SPECTRAL_GROUP_MAX 8
typedef struct {
    const float* w_bar;
    float* u;
    float* v;
    int R, C, T;
    float* t_out;
    float* sigma_out;
    void* w;
    void* wt;
} gcc_sn_item_t;
size_t gcc_spectral_group_workspace(const gcc_sn_item_t* items, int n);
int gcc_spectral_power_iteration_pack_group(const gcc_sn_item_t* items, int n, void* ws, size_t ws_bytes, gcc_stream_t stream);
int gcc_spectral_grad(const float* g_eff, const float* w_bar, const float* u, const float* v, const float* t_fwd,
                      const float* sigma_fwd, int R, int C, int T, float* dw_bar, float* du, float* dv, void* ws,
                      size_t ws_bytes, gcc_stream_t stream);
/* Eval-mode coefficients of the generator's spectrally normalised ConvTranspose2d + BatchNorm2d layers (SaganGeneratorEngine.infer):
 * the grouped power iteration of gcc_spectral_power_iteration_pack_group -- u, v, t_out and sigma_out the same bits -- in THREE
 * launches, the third of which (every workgroup of a layer forms the same sigma) also writes, for the C output channels,
 *     scale[c] = gamma[c] / (sigma sqrt(running_var[c] + eps))
 *     shift[c] = beta[c] + (bias[c] - running_mean[c]) gamma[c] / sqrt(running_var[c] + eps)
 * so that scale * conv(x, bf16(W_bar)) + shift is the eval-mode BatchNorm of the conv with W_bar / sigma and its bias (sigma does
 * not divide the bias).  No weight is written.  gamma / beta / bias / running_mean NULL: 1 / 0 / 0 / 0; running_var NULL: no
 * division by sqrt(running_var + eps).  Added without a GCC_HIP_ABI bump (additions only).  n <= GCC_SPECTRAL_GROUP_MAX;
 * ws: gcc_spectral_eval_coeffs_workspace(items, n) bytes (every layer its own scratch), 16-byte aligned. */
typedef struct {
    const float* w_bar;
    float* u;
    float* v;
    int R, C, T;
    float* t_out;
    float* sigma_out;
    const float* gamma; const float* beta; const float* running_mean; const float* running_var;
    const float* bias;
    float eps; int pad_;
    float* scale; float* shift;     /* [C] each */
} gcc_sn_eval_item_t;
size_t gcc_spectral_eval_coeffs_workspace(const gcc_sn_eval_item_t* items, int n);
int gcc_spectral_eval_coeffs_group(const gcc_sn_eval_item_t* items, int n, void* ws, size_t ws_bytes, gcc_stream_t stream);
/* Self attention, Self_Attn.forward (:72-104), per image over N = H*W <= 1024 positions: q, k (C8 channels) and v
 * (C <= 512 channels) are channel slices (qoff / koff / voff) of one NHWC bf16 buffer; y = gamma * softmax(q^T k) v + x.
 * The N x N score / attention matrices are never stored: the kernels recompute score tiles on the matrix cores (their
 * inner dimension is C/8).  Saved for backward: o (pre-gamma output, bf16 [B][N][ldo]) and stats (fp32 [B][N][2]: row
 * maximum and row sum of exp(s - max)).  A: optional fp32 [B][N][N] attention map -- the reference's forward returns it
 * (models/SAGAN.py:103), SAGANModel drops it; NULL skips the write.
 * gcc_attention_bwd: dq / dk / dv into the same slices of dqkv, dgamma (+=); rowdot is an fp32 [B][N] scratch.  The
 * residual branch (dx += dy) belongs to the caller. */
int gcc_attention_fwd(const void* qkv, int ldq, int qoff, int koff, int voff, const void* x, int ldx,
                      const float* gamma, int B, int N, int C, int C8, void* y, int ldy, void* o, int ldo,
                      float* stats, float* A, gcc_stream_t stream);
int gcc_attention_bwd(const void* qkv, int ldq, int qoff, int koff, int voff, const void* o, int ldo,
                      const float* stats, const float* gamma, const void* dy, int lddy, int B, int N, int C, int C8,
                      void* dqkv, int lddq, float* rowdot, float* dgamma, gcc_stream_t stream);
/* Eval-only self attention (SaganGeneratorEngine.infer): y = gamma * softmax(q^T k) v + x as gcc_attention_fwd, with ONE pass
 * over the keys (online softmax: running row maximum and sum, O rescaled in fp32) and nothing written but y -- no o, statistics
 * or map.  y = gamma * O / l + x is formed in fp32 and rounded to bf16 once; channels C .. ceil8(C) - 1 of y are written as
 * zeros.  K and V rows go through LDS once per workgroup.  Small grids (B = 1) split the keys over workgroups when `ws` holds
 * gcc_attention_infer_workspace() bytes (16-byte aligned): fp32 (m, l, O) partials, then a second launch folds them and applies
 * the epilogue; with ws NULL nothing is split.  Limits as gcc_attention_fwd (N <= 1024, C <= 512, 0 < C8 <= min(64, C)): any
 * other geometry returns GCC_ERR_UNSUPPORTED, a missing pointer or an ld / offset that is not a multiple of 8 (or ldq below
 * voff + ceil8(C), ldy below ceil8(C)) GCC_ERR_BAD_ARG, before anything is launched.  Added without a GCC_HIP_ABI bump.
 * gcc_attention_infer_route answers without launching: the launches the call makes with `ws_bytes` of workspace (1, or 2 when
 * the keys are split), or GCC_ERR_UNSUPPORTED.  gcc_attention_infer_workspace: 0 when the geometry is never split. */
int gcc_attention_infer(const void* qkv, int ldq, int qoff, int koff, int voff, const void* x, int ldx, const float* gamma,
                        int B, int N, int C, int C8, void* y, int ldy, void* ws, size_t ws_bytes, gcc_stream_t stream);
size_t gcc_attention_infer_workspace(int B, int N, int C, int C8);
int gcc_attention_infer_route(int B, int N, int C, int C8, size_t ws_bytes);
/* gcc_attention_infer_f32: gcc_attention_infer at the reference's own precision (SaganGeneratorEngine.infer, precision 'fp32';
 * gcc_amd/csrc/sagan_f32.hip).  q, k (C8 channels) and v (C channels) are fp32 channel slices of one NHWC fp32 buffer, x and y NHWC
 * fp32; both products run on v_mfma_f32_16x16x4_f32 (bit for bit k-ordered fmaf chains); the N x N matrices are never stored.
 * ONE launch: no key split, no workspace, no atomics, no workgroup waiting for another; an image alone and the same image inside a
 * batch give the same bits.  Added without a GCC_HIP_ABI bump (additions only).  The arithmetic contract:
 *     s_ij = the fmaf chain from 0 over the channels d = 0, 1, ... C8 - 1 of q_i[d] k_j[d] (zero padding to the instruction's K
 *            step adds exact zeros);  m_i = max_j s_ij;  p_ij = expf(s_ij - m_i) with the device library's expf
 *     l_i = sum_j p_ij,  O_ic = sum_j p_ij v_jc: fp32 fmaf chains from 0 (l_i: of p_ij x 1) in ONE order of the keys -- the tiles
 *            of 16 keys ascending, inside a tile key 4 g + r with r = 0..3 outer and g = 0..3 inner (0, 4, 8, 12, 1, 5, ...) --
 *            which depends on N alone: not on B, the grid, the tile a query fell into, or C.  O is never rescaled (two passes
 *            over the keys: the row maximum first, then l and O from recomputed scores)
 *     y_ic = fmaf(gamma, O_ic / l_i, x_ic), the division correctly rounded
 * Limits as gcc_attention_infer (N <= 1024, C <= 512, 0 < C8 <= min(64, C)), C a multiple of 8, any C8, B <= 65535:
 *   GCC_ERR_UNSUPPORTED otherwise.  ld and offsets in floats, multiples of 4, pointers 16-byte aligned, ldq >= voff + C (and
 *   >= qoff + C8, koff + C8), ldx >= C, ldy >= C; a null pointer or a bad ld / offset: GCC_ERR_BAD_ARG.  Every refusal happens
 *   before anything is launched.  Only channels [0, C) of y are written.
 * gcc_attention_infer_f32_route: 1 (the launches the call makes) or the geometry's error; launches nothing. */
int gcc_attention_infer_f32(const float* qkv, int ldq, int qoff, int koff, int voff, const float* x, int ldx,
                            const float* gamma, int B, int N, int C, int C8, float* y, int ldy, gcc_stream_t stream);
int gcc_attention_infer_f32_route(int B, int N, int C, int C8);
/* gcc_conv_eval_f32_z4: the SAGAN generator's first layer at the reference's own precision, ConvTranspose2d(Z, C, 4) on a 1 x 1
 * map: the GEMM [N, Z] x [Z, 16 C] on gcc_conv_eval_f32's tile (its matrix instruction and ONE order of K, walked in steps of 16,
 * every product an fmaf onto the running sum; no split-K, no atomics, no workspace: an image does not depend on its batch or
 * tile).  One launch.  Added without a GCC_HIP_ABI bump (additions only); the five entries on that tile keep their bits.
 *     y[n][kh][kw][c] = act(fmaf(acc, scale[c], shift[c]))      act: GCC_EVAL_ACT_NONE | _RELU; scale / shift NULL: 1 / 0
 * x: NHWC fp32 [N][1][1][ldx] (pointer to channel 0 of the Z channels), y: NHWC fp32 [N][4][4][ldy] (pointer to channel 0 of
 *   the C written ones); ld in floats, multiples of 4, ldx >= Z, ldy >= C, pointers 16-byte aligned.
 * Weights: fp32 [16 C][Kp], row (kh 4 + kw) C + c holding element [z][c][kh][kw] of ConvTranspose2d's [Z][C][4][4] at k = z,
 *   zeros from Z to Kp = gcc_conv_eval_f32_z4_kp(Z), the next multiple of 16.
 * Z a multiple of 4 (<= 2^20), C a multiple of 8 (<= 65536), N <= 2^24: GCC_ERR_UNSUPPORTED otherwise; a non-positive size, a
 *   null x / w / y, another act, a bad ld or alignment: GCC_ERR_BAD_ARG.  Every refusal happens before anything is launched.
 * gcc_conv_eval_f32_z4_route: the tile (0: 128 latents x 128 columns, 1: 64 x 64, chosen as the sibling entries do from N rows
 *   and 16 C columns -- the 32-column tile is never taken) or the geometry's error; launches nothing. */
int gcc_conv_eval_f32_z4(const float* x, int ldx, const float* w, const float* scale, const float* shift, int act, int N, int Z,
                         int C, float* y, int ldy, gcc_stream_t stream);
int gcc_conv_eval_f32_z4_route(int N, int Z, int C);
int gcc_conv_eval_f32_z4_kp(int Z);

/* ---------------------------------------------------------------------------------------------
 * SRGAN (models/SRGAN.py, models/GANLoss.py:95-145).
 * gcc_prelu: nn.PReLU() with its single learnable slope (device scalar), optionally fused with the nn.PixelShuffle(2)
 * in front of it (SubPixelConvolutionalBlock, :68-99): shuffle == 2 reads x [N][H][W][4C] and writes y [N][2H][2W][C],
 * y[n][2h+i][2w+j][c] = prelu(x[n][h][w][4c+2i+j]).  backward != 0: dx (layout of x) from dy (layout of y), and
 * dslope (+=, may be NULL: the distillation optimizer of the reference leaves the PReLU slopes out, :349-352); with a
 * workspace (GCC_PRELU_WORKSPACE_BYTES, zero-filled once by the caller, one per stream; its first 33 words -- the arrival counters -- are zero again after
 * every call) the sum behind dslope is formed in a fixed order -- bit-reproducible; without one (NULL) by atomic adds.
 * gcc_maxpool2x2: nn.MaxPool2d(2, 2) of the VGG stack; backward (1) routes to the first maximum in scan order; backward == 2: x is
 * the output of a ReLU and the ReLU's backward is applied on the way (a gradient whose maximum is not positive is dropped).
 * gcc_pool_linear_*: AdaptiveAvgPool2d((1,1)) + Linear(C, 1) of the discriminators (:245-262): pooled [N][C] fp32 is
 * kept for the backward pass, logit is bf16 [N][ldl] (one pixel per image, as gcc_gan_loss reads it).  gcc_pool_linear_bwd: dx, dw
 * (+=) and db (+=) may each be NULL; dw and db come out of one launch, whichever of them is asked for. */
int gcc_prelu(int backward, const void* x, int ldx, const float* slope, int C, int N, int H, int W, int shuffle,
              void* y, int ldy, const void* dy, int lddy, void* dx, int lddx, float* dslope, void* workspace,
              size_t workspace_bytes, gcc_stream_t stream);
#define GCC_PRELU_WORKSPACE_BYTES ((size_t)256 + 4 * 4096)
int gcc_maxpool2x2(int backward, const void* x, int ldx, void* y, int ldy, const void* dy, int lddy, void* dx, int lddx,
                   int N, int Ho, int Wo, int C, gcc_stream_t stream);
int gcc_pool_linear_fwd(const void* x, int ldx, int N, int HW, int C, const float* w, const float* b, float* pooled,
                        void* logit, int ldl, gcc_stream_t stream);
int gcc_pool_linear_bwd(const void* dlogit, int ldl, const float* w, const float* pooled, int N, int HW, int C,
                        void* dx, int lddx, float* dw, float* db, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer: multi-tensor Adam (torch.optim.Adam, no weight decay; models/Pix2Pix.py:382,415,
 * 430-431) with the L1-sparsity sub-gradient of L1_sparsity() (:554-563) fused in.
 * `tensors` / `chunks` are DEVICE arrays built once per optimizer; step is the 1-based step count.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float* p; const float* g; float* m; float* v;
    int64_t numel;
    float l1;        /* grad += l1 * sign(p) before the update (lambda_weight / lambda_scale) */
    float grad_scale;/* grad *= grad_scale first (1/world_size after a sum all-reduce) */
} gcc_adam_tensor_t;
/* work list: one 256-thread workgroup per chunk of `chunk_elems` consecutive elements of one tensor */
typedef struct { int tensor; int pad_; int64_t offset; } gcc_adam_chunk_t;
int gcc_adam_step(const gcc_adam_tensor_t* tensors, const gcc_adam_chunk_t* chunks, int nchunks, int chunk_elems,
                  float lr, float beta1, float beta2, float eps, int step, gcc_stream_t stream);

/* misc fp32 helpers */
/* device-side scalar algebra of the arch step (models/Pix2Pix.py:484-486, 505-511):
 * op 0: out = |a-b| ; op 1: out = k0*|a-b| + k1*c ; op 2: out = a + k0*b */
int gcc_scalar_op(int op, const float* a, const float* b, const float* c, float k0, float k1, float* out,
                  gcc_stream_t stream);
int gcc_fill_f32(float* p, float v, size_t n, gcc_stream_t stream);
int gcc_clamp_f32(float* p, float lo, float hi, size_t n, gcc_stream_t stream);
/* dst[i] += src[i]: folds a gradient accumulated apart (the architecture step's second discriminator pass, run beside the first
 * on another stream: models/Pix2Pix.py:496-511 accumulates both into DifferentiableOP.alpha.grad) in the reference's order */
int gcc_add_f32(float* dst, const float* src, size_t n, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation arithmetic.  The evaluator networks (Inception, DRN) stay external: these entry
 * points take their outputs as device tensors.
 * gcc_argmax_channels: scores NCHW fp32 [N][C][HW] -> class index int32 [N][HW], numpy.argmax semantics
 *   (metric/mIoU_score.py:212 `final.argmax(axis=1)`).
 * gcc_confusion_hist: fast_hist (metric/mIoU_score.py:163-167): hist[n * label + pred] += 1 where 0 <= label < n; int64
 *   [n][n], accumulated (+=) so that a whole evaluation set sums into one matrix.  Exact.
 * gcc_psnr_y_sse: sum of squared luminance differences of two NCHW fp32 images in [-1, 1] with the 4-pixel border
 *   cropped (models/SRGAN.py:653-657: convert_image(..., 'y-channel'), data/sr_dataset.py:36-37, 58-62); PSNR =
 *   10 log10(255^2 N (H-8)(W-8) / sse).  f64 accumulation in a fixed order.
 * gcc_ssim_y_sum: sum over the N images and over all window centres of the SSIM map of the same luminance images
 *   (models/SRGAN.py:659-661, skimage.metrics.structural_similarity(real_y, fake_y, data_range=255.) with its defaults: 7 x 7
 *   uniform window, K1 = .01, K2 = .03, sample covariance, border of 3 cropped); SSIM = sum / (N (H-14)(W-14)).  f64.
 *   Workspace as gcc_psnr_workspace().  (skimage is an un-pinned dependency that the build image lacks: parity unpinned.)
 * gcc_activation_stats: mu = mean(act, 0), sigma = np.cov(act, rowvar=False) in f64 (metric/fid_score.py:327-328) of
 *   activations [n][d] (fp32 or f64, row major).
 * gcc_frechet_distance: metric/fid_score.py:219-284; out[0] = |mu1-mu2|^2 + tr(s1) + tr(s2) - 2 tr(sqrtm(s1 s2)) with
 *   the matrix square root by `iterations` coupled Newton-Schulz steps on the GPU (f64) of s1 s2 + delta I, delta =
 *   shift_rel |s1 s2|_F, solved at delta and 4 delta and extrapolated to delta = 0 (shift_rel = 0: one unshifted solve,
 *   full-rank inputs only); out[1] = relative change of the trace over the last step (the caller's convergence check).
 * --------------------------------------------------------------------------------------------- */
int gcc_argmax_channels(const float* scores, int N, int C, size_t HW, int* pred, gcc_stream_t stream);
int gcc_confusion_hist(const int* pred, const int* label, size_t count, int n, long long* hist, gcc_stream_t stream);
size_t gcc_psnr_workspace(void);
int gcc_psnr_y_sse(const float* fake, const float* real, int N, int H, int W, double* sse, int accumulate, void* ws,
                   size_t ws_bytes, gcc_stream_t stream);
int gcc_ssim_y_sum(const float* fake, const float* real, int N, int H, int W, double* ssim_sum, int accumulate, void* ws,
                   size_t ws_bytes, gcc_stream_t stream);
size_t gcc_activation_stats_workspace(int n, int d);
int gcc_activation_stats(const void* act, int is_f64, int n, int d, double* mu, double* sigma, void* ws, size_t ws_bytes,
                         gcc_stream_t stream);
size_t gcc_frechet_workspace(int d);
int gcc_frechet_distance(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2, int d,
                         int iterations, double shift_rel, double* out, void* ws, size_t ws_bytes, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input pipeline (data/aligned_dataset.py:27-56, data/base_dataset.py:63-112) on decoded
 * 8-bit RGB images in device memory ([H][W][3] rows of `pitch` bytes; a half of the paired A|B image is addressed by
 * offsetting `src`).
 * gcc_resample_u8: PIL's Image.resize(..., BICUBIC) -- any of its separable filters, the coefficient tables decide --
 *   bit for bit: horizontal pass, uint8 intermediate, vertical pass, 22-bit fixed-point coefficients (hcoef [out_w][hk],
 *   hbounds [out_w][2] = first source column and tap count; likewise v*), tmp = in_h * out_w * 3 bytes when both passes
 *   run.  dst is tightly packed [out_h][out_w][3].
 * gcc_crop_flip_normalize: __crop + __flip + ToTensor + Normalize((.5,.5,.5),(.5,.5,.5)): NCHW fp32 [3][crop_h][crop_w]
 *   and / or the NHWC bf16 model input (pixel stride ld, channels 0..2 written).
 * --------------------------------------------------------------------------------------------- */
int gcc_resample_u8(const void* src, int in_h, int in_w, size_t pitch, void* dst, int out_h, int out_w, const int* hbounds,
                    const int* hcoef, int hk, const int* vbounds, const int* vcoef, int vk, void* tmp, gcc_stream_t stream);
int gcc_crop_flip_normalize(const void* src, int H, int W, size_t pitch, int x0, int y0, int crop_h, int crop_w, int flip,
                            float* nchw, void* nhwc_bf16, int ld, gcc_stream_t stream);
/* the same with the range conversion chosen: form 0 Normalize(mean3, std3) (host arrays; ImageNet statistics for the SRGAN
 * low-resolution input, data/sr_dataset.py:52-56), form 1 convert_image '[-1, 1]' = 2 (v / 255) - 1 (:49-50), form 2 v / 255 */
int gcc_crop_convert(const void* src, int H, int W, size_t pitch, int x0, int y0, int crop_h, int crop_w, int flip, int form,
                     const float* mean3, const float* std3, float* nchw, void* nhwc_bf16, int ld, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Cityscapes mIoU around the segmenter (metric/test_metric.py:47-87, metric/mIoU_score.py:70-105, 169-218).  Added without a
 * GCC_HIP_ABI bump (additions only).
 * gcc_seg_input: the segmenter's input from the generator's output in one launch: NCHW fp32 out[N][3][H][W] =
 *   (float(byte) / 255.f - mean3[c]) / std3[c] in fp32 with two IEEE divisions (SegList's ToTensor + Normalize), where byte is
 *   util.tensor2im's byte exactly as gcc_image_to_u8 computes it from an NHWC bf16 image [N][H][W] (ld, off: multiples of 8), or,
 *   with is_u8 != 0, the byte itself of a DEVICE uint8 [N][H][W][3] image (ld, off unused).  mean3 / std3: host arrays.
 * gcc_miou_score: resize_4d_tensor(final, W, H).argmax(axis=1) followed by fast_hist, per output pixel, without the resized
 *   tensor.  scores NCHW fp32 [N][C][h][w]; labels uint8 [N][H][W]; the tables are Pillow's precompute_coeffs for BILINEAR in
 *   double precision (not normalised to fixed point): hbounds int32 [W][2] = first source column and tap count, hcoef f64
 *   [W][hk]; vbounds [H][2], vcoef [H][vk].  Resample.c for 32-bit float images: horizontal pass first, ss = 0.0;
 *   ss += (double)src * coef per tap in tap order (an f64 multiply, then an f64 add: never fused), every tap inside the bounds
 *   multiplied whatever its coefficient, the sum rounded to fp32; then the vertical pass over those fp32 values likewise.  A
 *   pass PIL skips (equal sizes) has the one-coefficient table {1.0}: 0.0 + v * 1.0 is v for the argmax (-0.0 becomes +0.0,
 *   which compares equal; the resized value itself is never output).  argmax as gcc_argmax_channels.  hist[C * label + pred]
 *   += 1 where label < C (int64 [C][C], accumulated); pred: optional uint8 [N][H][W] (NULL: not written).  Supported: h <= H,
 *   w <= W, hk <= 3, vk <= 3, C <= 64; GCC_ERR_UNSUPPORTED otherwise, before anything is launched.  Indices read from the
 *   tables are clamped into the source plane: a malformed table gives wrong numbers, never an access outside `scores`.
 * --------------------------------------------------------------------------------------------- */
int gcc_seg_input(const void* x, int is_u8, int ld, int off, int N, int H, int W, const float* mean3, const float* std3,
                  float* out, gcc_stream_t stream);
int gcc_miou_score(const float* scores, int N, int C, int h, int w, const unsigned char* labels, int H, int W, const int* hbounds,
                   const double* hcoef, int hk, const int* vbounds, const double* vcoef, int vk, long long* hist,
                   unsigned char* pred, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The segmenter itself (DRN-D of metric/drn.py under DRNSeg, metric/mIoU_score.py:124-157): its convolutions are
 * gcc_conv_eval_ex / gcc_conv_fprop_eval calls; these are the three streaming pieces around them (gcc_amd/csrc/segnet.hip,
 * gcc_amd/metric/drn_seg.py).  Added without a GCC_HIP_ABI bump (additions only).  One launch each unless stated; every refusal
 * happens before anything is launched.
 * gcc_phase_regroup: "phase layout" d of a logical NHWC bf16 image [N][H][W] is the image [N d^2][H / d][W / d] in which logical
 *   pixel (n, h, w) sits at batch index n d^2 + (h mod d) d + (w mod d), row h div d, column w div d (d = 1: the image itself).
 *   A 3 x 3, stride-1 convolution of dilation d and zero padding d of the logical image is the plain 3 x 3, padding-1
 *   convolution of its phase layout d.  The call copies channels [soff, soff + C) of `src` (layout d_src) to channels
 *   [doff, doff + C) of `dst` (layout d_dst) in 16-byte chunks; channels [C, ceil8(C)) of the destination window are written as
 *   zeros, every other channel of dst is left alone.  GCC_ERR_BAD_ARG: a null pointer, a non-positive size, an ld / offset that
 *   is no multiple of 8, a window that does not fit its ld, buffers that overlap (the permutation is not done in place);
 *   GCC_ERR_UNSUPPORTED: a d other than 1, 2, 4, or H / W that are no multiples of both.
 * gcc_relu_bf16: x[p][off + c] = x > 0 ? x : +0 in place for c < C, p < pixels (NaN stays NaN, -0 becomes +0): the ReLU of
 *   relu(bn(conv) + residual) behind gcc_conv_fprop_eval.  Channels outside the window are untouched.
 * gcc_seg_head: DRNSeg's output end in fp32, two launches.
 *   (a) x != NULL: scores[n][c][p] = seg_b[c] + sum_k seg_w[c][k] x[n][p][off + k], the 1 x 1 `seg` conv of the NHWC bf16 feature
 *       map x [N][h][w] (Cin channels, a multiple of 8; seg_w fp32 [C][Cin]; seg_b fp32 [C] or NULL), NCHW fp32 [N][C][h][w].
 *       x == NULL: `scores` is read as given.
 *   (b) logp != NULL: logp = LogSoftmax_c(ConvTranspose2d(C, C, 16, stride 8, padding 4, groups C, no bias)(scores)) with the
 *       weights up_w fp32 [C][1][16][16] (read, never assumed bilinear), NCHW fp32 [N][C][8h][8w]; at most 2 x 2 taps reach an
 *       output pixel, whose C values stay in one thread's registers.
 *   C <= 64, GCC_ERR_UNSUPPORTED beyond.
 * gcc_seg_head_f32: the same two launches with x an NHWC FP32 feature map (ld, off in floats, multiples of 4): the output end of
 *   the fp32 route (gcc_conv_eval_f32).  Same sums in the same order; x == NULL is gcc_seg_head's x == NULL.
 * --------------------------------------------------------------------------------------------- */
int gcc_phase_regroup(const void* src, int lds, int soff, int d_src, void* dst, int ldd, int doff, int d_dst, int N, int H, int W,
                      int C, gcc_stream_t stream);
int gcc_relu_bf16(void* x, int ld, int off, int C, size_t pixels, gcc_stream_t stream);
int gcc_seg_head(const void* x, int ld, int off, int N, int h, int w, int Cin, const float* seg_w, const float* seg_b, int C,
                 const float* up_w, float* scores, float* logp, gcc_stream_t stream);
int gcc_seg_head_f32(const float* x, int ld, int off, int N, int h, int w, int Cin, const float* seg_w, const float* seg_b, int C,
                     const float* up_w, float* scores, float* logp, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The FID Inception-v3 network (metric/inception.py:166-315 fid_inception_v3 under InceptionV3([3])): its convolutions are
 * gcc_conv_eval_ex calls; these are the streaming pieces around them (gcc_amd/csrc/inception.hip,
 * gcc_amd/metric/inception_fid.py).  Added without a GCC_HIP_ABI bump (additions only).  One launch each, 16-byte accesses over
 * 8-channel chunks, no atomics; every refusal happens before anything is launched: GCC_ERR_BAD_ARG for a null pointer, a
 * non-positive size, an ld / offset that is no multiple of 8, a window that does not fit its ld, a pointer off its alignment;
 * GCC_ERR_UNSUPPORTED for a channel count that is no multiple of 8.
 * gcc_fid_resize: y[n][oy][ox][off + c] = bf16(2 v - 1), v = F.interpolate(x, (Ho, Wo), mode = 'bilinear', align_corners =
 *   False) of the NCHW fp32 image x [N][3][H][W], in fp32 with torch's source index max(0, (o + 0.5) (in / out) - 0.5), the
 *   upper neighbour clamped to in - 1 (it enlarges and shrinks; no antialiasing); channels off + 3 .. off + 7 are written as
 *   zeros.  y: NHWC bf16 [N][Ho][Wo], ld elements per pixel.
 * gcc_pool3x3: 3 x 3 pooling of channels [xoff, xoff + C) of the NHWC bf16 map x [N][H][W] into channels [yoff, yoff + C) of y;
 *   every other channel of y is left alone.  GCC_POOL3_MAX_S2: max, stride 2, no padding, y [N][(H - 3) / 2 + 1][(W - 3) / 2 +
 *   1] (H, W >= 3); GCC_POOL3_MAX_S1P1: max, stride 1, padding 1 of -inf, y [N][H][W]; GCC_POOL3_AVG_S1P1: mean over the taps
 *   inside the map (count_include_pad = False), fp32 sum, one division, one rounding.  x and y must not overlap.
 * gcc_border_copy: dst [N][H + 2 ph][W + 2 pw] = src [N][H][W] with a border of ph rows and pw columns of zeros around it, for
 *   channels [soff, soff + C) -> [doff, doff + C); the border is written in the same launch whatever dst held.  A convolution with
 *   a (KH, KW) kernel and padding (ph, pw) of src is the padding-0 convolution of dst.  Never in place (GCC_ERR_BAD_ARG).
 * gcc_global_avgpool: out[n][c] = mean over the h w pixels of x[n][.][off + c], fp32 [N][C] (16-byte aligned), summed in fp32
 *   in an order the shape alone fixes (eight interleaved partial sums, then a tree).
 * --------------------------------------------------------------------------------------------- */
#define GCC_POOL3_MAX_S2 0
#define GCC_POOL3_MAX_S1P1 1
#define GCC_POOL3_AVG_S1P1 2
int gcc_fid_resize(const float* x, int N, int H, int W, void* y, int ld, int off, int Ho, int Wo, gcc_stream_t stream);
int gcc_pool3x3(int mode, const void* x, int ldx, int xoff, void* y, int ldy, int yoff, int N, int H, int W, int C,
                gcc_stream_t stream);
int gcc_border_copy(const void* src, int lds, int soff, void* dst, int ldd, int doff, int N, int H, int W, int C, int ph, int pw,
                    gcc_stream_t stream);
int gcc_global_avgpool(const void* x, int ld, int off, int N, int h, int w, int C, float* out, gcc_stream_t stream);
/* The same three kernels on NHWC FP32 maps, around gcc_conv_eval_f32_ex (the network at the reference's own precision): the same
 * arithmetic in the same order without the bf16 roundings.  A 16-byte chunk is 4 channels: ld / offsets multiples of 4 floats,
 * C a multiple of 4 (GCC_ERR_UNSUPPORTED otherwise); the refusals are the bf16 entries' otherwise, all before any launch.  There
 * is no fp32 border copy: rectangular padding is gcc_conv_eval_f32_ex's own index arithmetic.
 * gcc_fid_resize_f32: y[n][oy][ox][off + c] = 2 v - 1 for c < 3, and channel off + 3 is written as zero (the 3-in-4 input of
 *   gcc_conv_eval_f32_ex with Ci == 3).  The source index (o + 0.5) (in / out) - 0.5 is one fused multiply-add on the fp32
 *   ratio of the sizes, in both entries: what torch's fp32 builds compute (a float64 index differs by up to 7e-5 in v).
 * gcc_pool3x3_f32: the maxima are the inputs' own bits (of equal maxima the first met, a NaN wins); the average is the fp32 sum
 *   in tap order (row by row, left to right) over the taps inside the map, then one IEEE division by their count.
 * gcc_global_avgpool_f32: pixel p goes to partial sum p mod 8, the partials are added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 +
 *   7)), then one IEEE division by h w. */
int gcc_fid_resize_f32(const float* x, int N, int H, int W, float* y, int ld, int off, int Ho, int Wo, gcc_stream_t stream);
int gcc_pool3x3_f32(int mode, const float* x, int ldx, int xoff, float* y, int ldy, int yoff, int N, int H, int W, int C,
                    gcc_stream_t stream);
int gcc_global_avgpool_f32(const float* x, int ld, int off, int N, int h, int w, int C, float* out, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The spatial mean of a LARGE map: the network's earlier output blocks (metric/inception.py BLOCK_INDEX_BY_DIM: 64 channels at
 * 73 x 73, 192 at 35 x 35, 768 at 17 x 17 for a 299 x 299 input), averaged to 1 x 1 as metric/fid_score.py:136-137 does
 * (gcc_amd/csrc/inception.hip, InceptionFidEngine(output_blocks=, pooled=True)).  Added without a GCC_HIP_ABI bump (additions
 * only); gcc_global_avgpool(_f32) keep their behaviour and their bits.
 * Operand.  x is an NHWC channel window as in gcc_global_avgpool: bf16 in 16-byte chunks of 8 channels (gcc_map_mean) or fp32 in
 *   chunks of 4 (gcc_map_mean_f32), C a multiple of the chunk, ld and off on the chunk grid with ld >= off + C, x 16-byte
 *   aligned.  Nothing between off + C and ld, or after the last pixel, is read.  out: fp32 [N][C], 16-byte aligned.
 * Result.  out[n * C + c] = (float)(S / (double)(h w)), S the sum of the h w values x[n][.][off + c], each converted to f64
 *   (exactly) and accumulated in f64: one division in f64, then one rounding to fp32.  Whatever the order, |S_computed - S| <=
 *   gamma_{h w} sum |x| (gamma_n = n u / (1 - n u), u = 2^-53); a map of integers below 2^53 / (h w) in magnitude is summed
 *   exactly, so every `segments` gives it the same bits.
 * Order.  The pixels of an image are cut into `segments` ranges (range s is [s P / segments, (s + 1) P / segments), P = h w);
 *   a workgroup owns one range of one image for a block of CW chunks (CW: the largest power of two that divides C / chunk, at most
 *   256 / chunk channels), its 256 threads as R = 256 / CW pixel rows: row r adds pixels lo + r, lo + r + R, ... in ascending
 *   order, eight 16-byte loads in flight; the rows are added through LDS in ascending r, the ranges in ascending s.  The order
 *   is a function of h w, C and `segments` alone -- not of N, of the image's place in the batch, of ld or off -- so an image's
 *   mean does not depend on its batch neighbours, bit for bit.
 * segments == 0: the library's split gcc_map_mean_segments(h, w, C) = clamp(P / ((256 / CW4) GCC_MAP_MEAN_PIXELS_PER_THREAD), 1,
 *   max) with CW4 the CW of C / 4 chunks for either element type: a function of h w and C alone.  1 <= segments <= max = min(h w,
 *   GCC_MAP_MEAN_MAX_SEGMENTS) forces it (for tests).  gcc_map_mean_segments is 0 for a size < 1 or a C that is no multiple of 4.
 * Execution.  segments in use == 1: one launch, nothing is written to ws (ws may be NULL).  Otherwise the per-range sums go to ws
 *   as f64 [N][segments][C] and a second launch adds them: two launches.  No floating-point atomics, no workgroup waits for
 *   another, nothing is zero-filled: the same input gives the same bits.
 * gcc_map_mean_workspace(N, h, w, C): bytes that serve every legal `segments` (N max C doubles); 0 for a size < 1.
 * Refusals, all before anything is launched: GCC_ERR_BAD_ARG for a null x or out (or ws with more than one range in use), a size
 *   < 1, an ld / off off the chunk grid, ld < off + C, a pointer off its alignment (ws: 8 bytes), segments < 0 or above max;
 *   GCC_ERR_UNSUPPORTED for a C that is no multiple of the chunk, h w >= 2^24, N h w ld >= 2^40 (gcc_global_avgpool's limits) or
 *   2^31 workgroups; GCC_ERR_WORKSPACE for ws_bytes short of N segments C doubles with more than one range in use.
 * --------------------------------------------------------------------------------------------- */
#define GCC_MAP_MEAN_MAX_SEGMENTS 64
#define GCC_MAP_MEAN_PIXELS_PER_THREAD 64
int gcc_map_mean_segments(int h, int w, int C);
size_t gcc_map_mean_workspace(int N, int h, int w, int C);
int gcc_map_mean(const void* x, int ld, int off, int N, int h, int w, int C, int segments, float* out, void* ws, size_t ws_bytes,
                 gcc_stream_t stream);
int gcc_map_mean_f32(const float* x, int ld, int off, int N, int h, int w, int C, int segments, float* out, void* ws,
                     size_t ws_bytes, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FID around the Inception network (metric/test_metric.py:15-45, 129-204, metric/get_real_stat.py; the network itself is the
 * caller's).  Added without a GCC_HIP_ABI bump (additions only).
 * gcc_fid_input: the network's input, NCHW fp32 out[N][3][H][W] in [0, 1] = float(byte) / 255.f (equal to the reference's
 *   float(double(byte) / 255.0) for all 256 bytes), written at `out` (a slot of a batch buffer works), from
 *     GCC_FID_IN_BF16  an NHWC bf16 image [N][H][W] (ld, off: multiples of 8): byte as gcc_image_to_u8 / util.tensor2imgs
 *     GCC_FID_IN_U8    a DEVICE uint8 [N][H][W][3] image: the byte itself (ld, off unused)
 *     GCC_FID_IN_F32   an NCHW fp32 image in [-1, 1] (what the data loaders yield; ld, off unused): byte = trunc(clip((x + 1) / 2
 *                      * 255, 0, 255)) in fp32 in exactly that order -- 63 of the 256 bytes b do not come back from the loaders'
 *                      (b / 255 - 0.5) / 0.5 as b but as b - 1, and the real-image statistics are those of the reference only
 *                      when that is reproduced.
 * Streamed activation statistics: what gcc_activation_stats computes, from batches, with a workspace that does not grow with n.
 *   The caller keeps mean [d] and m2 [d][d] (f64, device) and the count of rows merged so far (a host integer).
 *   gcc_activation_stats_update merges b >= 1 rows act[b][d] (fp32 or f64, row stride ld >= d elements: a [b][d][1][1] network
 *   output is read in place): m_b = batch mean, Xc = batch - m_b, delta = m_b - mean,
 *       m2 += Xc^T Xc + (n_before b / (n_before + b)) delta delta^T ;  mean += delta b / (n_before + b)      (Chan et al.)
 *   in f64, two launches, fixed summation order.  n_before == 0: mean and m2 are written without being read (no zero fill
 *   needed).  ws: gcc_activation_stats_stream_workspace(max_batch, d) bytes serve every b <= max_batch; one stream at a time.
 *   gcc_activation_stats_finish: sigma = m2 / (n - 1) (sigma may be m2); GCC_ERR_BAD_ARG for n < 2.
 *   Both refuse (GCC_ERR_BAD_ARG / GCC_ERR_WORKSPACE) before anything is launched.
 * --------------------------------------------------------------------------------------------- */
enum { GCC_FID_IN_BF16 = 0, GCC_FID_IN_U8 = 1, GCC_FID_IN_F32 = 2 };
int gcc_fid_input(const void* x, int form, int ld, int off, int N, int H, int W, float* out, gcc_stream_t stream);
size_t gcc_activation_stats_stream_workspace(int max_batch, int d);
int gcc_activation_stats_update(const void* act, int is_f64, int ld, int b, int d, long long n_before, double* mean, double* m2,
                                void* ws, size_t ws_bytes, gcc_stream_t stream);
int gcc_activation_stats_finish(const double* m2, long long n, int d, double* sigma, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel Inception Distance (Binkowski et al. 2018) on the same activations (gcc_amd/csrc/kid.hip, gcc_amd/metric/kid_score.py).
 * Added without a GCC_HIP_ABI bump (additions only).
 * gcc_kid_poly_sum: out[0] = sum over pairs (i, j) of k(x_i, y_j), k = t t t with t = dot(x_i, y_j) (1.0 / d) + 1.0, all in f64.
 *   X [m][ldx], Y [n][ldy]: fp32 (x_f64 / y_f64 == 0) or f64 rows of d elements, row stride ld >= d elements; what lies between
 *   d and ld, or after the last row, is never read.  symmetric != 0: Y is X (the Y-side arguments are not read) and only the
 *   pairs i != j count; m >= 2.  Any m, n, d >= 1: nothing needs to be a multiple of the tile or the k-step.
 *   One workgroup per GCC_KID_TILE x GCC_KID_TILE tile of pairs (symmetric: the tiles on and above the diagonal, those above
 *   it counted twice) walks d in steps of GCC_KID_KSTEP and writes one f64 partial to ws; a second launch folds the partials in
 *   an order fixed by the tile index.  The m x n matrix is never stored: ws holds gcc_kid_workspace(m, n, d) bytes = one double
 *   per tile.  No floating-point atomics, no workgroup waits for another: the same input gives the same bits.  Two launches.
 *   GCC_ERR_BAD_ARG (a null pointer, a size < 1, ld < d, symmetric with m < 2), GCC_ERR_WORKSPACE (ws_bytes short) and
 *   GCC_ERR_UNSUPPORTED (2^31 tiles or more) are returned before anything is launched.
 * --------------------------------------------------------------------------------------------- */
#define GCC_KID_TILE 128
#define GCC_KID_KSTEP 16
size_t gcc_kid_workspace(int m, int n, int d);
int gcc_kid_poly_sum(const void* X, int x_f64, int ldx, int m, const void* Y, int y_f64, int ldy, int n, int d, int symmetric,
                     double* out, void* ws, size_t ws_bytes, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) on the same activations: the pairwise
 * half (gcc_amd/csrc/prdc.hip, gcc_amd/metric/prdc_score.py).  Added without a GCC_HIP_ABI bump (additions only).
 * Rows are given as in gcc_kid_poly_sum: fp32 (*_f64 == 0) or f64 rows of d elements, row stride ld >= d elements; what lies
 * between d and ld, or after the last row, is never read.  Any m, n, d >= 1.
 * The distance.  D(x, y) = sum_c (x_c - y_c)^2 in f64, the DIFFERENCE form: t = x_c - y_c (fp32 inputs are converted first,
 *   exactly), acc = fma(t, t, acc), for c = 0, 1, ..., d - 1 in this order from acc = +0: one chain of d subtractions and d fused
 *   multiply-adds per pair, two roundings per element.  Hence D >= 0, D(x, x') == 0 exactly for equal rows, D(x, y) == D(y, x)
 *   bit for bit, |D_computed - D| <= gamma_{d+2} D (relative to D itself, gamma_n = n u / (1 - n u), u = 2^-53: the subtraction's
 *   rounding enters squared, every term is non-negative and passes at most d additions), and the bits of D(i, j) are a function
 *   of the two rows and d alone -- not of where they sit in X / Y, of m, n, k, of `chunks` or of the tile.
 * gcc_prdc_kth_dist: out[i] (f64, i < m) = the k-th smallest over j < n of D(x_i, y_j).  symmetric != 0: Y is X (the Y-side
 *   arguments are not read) and j == i is left out.  1 <= k <= GCC_PRDC_MAX_K, and k <= n (symmetric: k <= m - 1).
 * gcc_prdc_ball_count: out[j] (int, j < m) = #{ i < n : D(q_j, c_i) <= r2[i] }; r2: n f64 squared radii.  <= is inclusive.
 * A workgroup owns T rows and walks one of `chunks` ranges of T-column tiles (range c of the N = ceil(n / T) column tiles is
 *   [c N / chunks, (c + 1) N / chunks)), d in steps of GCC_PRDC_KSTEP; the distances are consumed in registers and never stored:
 *   ws receives, per row and chunk, the k smallest so far (k doubles) or a count (one int), and a second launch merges them per
 *   row.  T, rows and columns alike, is GCC_PRDC_TILE (= GCC_PRDC_COL_TILE) where that tile can give every compute unit a
 *   workgroup -- ceil(m / 128) min(ceil(n / 128), GCC_PRDC_MAX_CHUNKS) >= GCC_PRDC_SMALL_BELOW -- and GCC_PRDC_SMALL_TILE below:
 *   a quarter of the work per workgroup and four times the workgroups for the sets of 120 to 1000 images this project scores.
 *   gcc_prdc_tile(m, n) says which; `tile` == 0 takes it, either constant forces it (for tests).  chunks == 0: the library's
 *   choice gcc_prdc_chunks(m, n) = min(ceil(GCC_PRDC_FILL_WORKGROUPS / ceil(m / T)), N, GCC_PRDC_MAX_CHUNKS) at T =
 *   gcc_prdc_tile(m, n) (with `tile` forced: the same formula at that tile), a function of (m, n) alone; 1 <= chunks <= min(N,
 *   GCC_PRDC_MAX_CHUNKS) forces it.  The k smallest of a multiset and a sum of integers do not depend on order, and both tiles
 *   run the same chain per pair: every legal `chunks` and either tile give the same bits.  No floating-point atomics, no
 *   workgroup waits for another: the same input gives the same bits.  Two launches each.
 * gcc_prdc_workspace(m, n, k): bytes that serve either entry at m rows against n at any legal `chunks` and `tile` (m min(ceil(n
 *   / GCC_PRDC_SMALL_TILE), GCC_PRDC_MAX_CHUNKS) k doubles; ball_count needs no more than k = 1); 0 for a size < 1 or k outside
 *   1..GCC_PRDC_MAX_K.
 * GCC_ERR_BAD_ARG (a null pointer, a size < 1, ld < d, k out of range or above the number of admissible j, a `tile` that is
 *   neither constant nor 0, `chunks` negative or above what n and the tile admit), GCC_ERR_WORKSPACE (ws_bytes short of what the
 *   chunks in use need) and GCC_ERR_UNSUPPORTED (2^31 workgroups or more) are returned before anything is launched.
 * --------------------------------------------------------------------------------------------- */
#define GCC_PRDC_TILE 128
#define GCC_PRDC_COL_TILE 128
#define GCC_PRDC_SMALL_TILE 64
#define GCC_PRDC_SMALL_BELOW 256
#define GCC_PRDC_KSTEP 16
#define GCC_PRDC_MAX_K 8
#define GCC_PRDC_MAX_CHUNKS 16
#define GCC_PRDC_FILL_WORKGROUPS 512
size_t gcc_prdc_workspace(int m, int n, int k);
int gcc_prdc_tile(int m, int n);
int gcc_prdc_chunks(int m, int n);
int gcc_prdc_kth_dist(const void* X, int x_f64, int ldx, int m, const void* Y, int y_f64, int ldy, int n, int d, int symmetric,
                      int k, int chunks, int tile, double* out, void* ws, size_t ws_bytes, gcc_stream_t stream);
int gcc_prdc_ball_count(const void* Q, int q_f64, int ldq, int m, const void* C, int c_f64, int ldc, int n, int d,
                        const double* r2, int chunks, int tile, int* out, void* ws, size_t ws_bytes, gcc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Inception Score (Salimans et al. 2016) on the same activations: the network's classifier head and the per-split scores
 * (gcc_amd/csrc/inception_score.hip, gcc_amd/metric/inception_score.py).  Added without a GCC_HIP_ABI bump (additions only).
 * X [n][ldx]: fp32 (x_f64 == 0) or f64 rows of d elements, row stride ldx >= d elements; what lies between d and ldx, or after
 * the last row, is never read.  W [C][d] and b [C]: fp32, contiguous.  Any n, d >= 1 and C >= 2; nothing needs to be a multiple
 * of the tile, the k-step or the chunk.  All arithmetic is f64.
 * gcc_is_logits: Z[i][c] (f64, [n][C] contiguous) = b[c] + sum_k X[i][k] W[c][k], as ONE chain per element: acc = b[c], then acc =
 *   fma(X[i][k], W[c][k], acc) for k = 0, 1, ..., d - 1 (and fma(0, 0, acc) up to the next multiple of GCC_IS_KSTEP): the bits of
 *   Z[i][c] are a function of row i, class c and d alone -- a row alone gives the bits it has in its set, at every `chunk`.
 * gcc_is_split_scores: scores[s] (f64, s < splits) of split s = rows [s n / splits, (s + 1) n / splits) (integer divisions: the
 *   original code's slicing), n_s of them.  Per row: m = max_c z_c, S = sum_c exp(z_c - m), logp_c = (z_c - m) - log S, p_c =
 *   exp(logp_c), h_i = sum_c p_c logp_c where a class with p_c == 0 adds exactly 0.  Per split: mbar_c = (sum_i p_ic) / n_s,
 *   KL = (sum_i h_i) / n_s - sum_c mbar_c log mbar_c (zero terms skipped), scores[s] = exp(KL).  The mean and the population
 *   standard deviation of the scores are the host's.
 * Rows go through in chunks of `chunk` (0: GCC_IS_CHUNK; any positive value forces it), three launches per chunk -- logits by
 *   GCC_IS_TILE x GCC_IS_TILE tiles over d in steps of GCC_IS_KSTEP, one wave per row, one thread per (split, class) -- and one
 *   launch at the end.  ws holds one chunk of logits / probabilities and [splits][C] + [splits] doubles of state carried from
 *   chunk to chunk: gcc_is_workspace(C, splits, chunk) = (chunk C + chunk + splits C + splits) doubles, whatever n is (0 for C <
 *   2, splits < 1 or chunk < 0).  Order of sums: a row's sums take lane l's classes l, l + 64, ... ascending and fold the lanes
 *   by xor-shuffles; a split's sums over rows are ONE chain in row order per class, which a chunk edge only interrupts; the sum
 *   over classes takes thread t's classes t, t + 256, ... and folds lanes, then waves.  Every order is fixed by (n, C, splits):
 *   the same input gives the same bits, at every `chunk`.  No floating-point atomics, no workgroup waits for another.
 * GCC_ERR_BAD_ARG (a null pointer, n or d < 1, C < 2, ldx < d, chunk < 0, splits < 1, n < splits), GCC_ERR_UNSUPPORTED (2^31
 *   workgroups or more) and GCC_ERR_WORKSPACE (ws_bytes short) are returned before anything is launched.
 * --------------------------------------------------------------------------------------------- */
#define GCC_IS_TILE 64
#define GCC_IS_KSTEP 16
#define GCC_IS_CHUNK 4096
size_t gcc_is_workspace(int C, int splits, int chunk);
int gcc_is_logits(const void* X, int x_f64, int ldx, int n, int d, const float* W, const float* b, int C, int chunk, double* Z,
                  gcc_stream_t stream);
int gcc_is_split_scores(const void* X, int x_f64, int ldx, int n, int d, const float* W, const float* b, int C, int splits,
                        int chunk, double* scores, void* ws, size_t ws_bytes, gcc_stream_t stream);

/* ---- gradient exchange ---------------------------------------------------------------------------------
 * The reference trains on one device (models/Pix2Pix.py:356); the data-parallel path sums the five optimizers' flat fp32
 * gradient buffers over ranks before each `optimizer.step()` (train.py has no counterpart: this is the exchange a
 * multi-GPU launch of it needs).  An explicit communicator over RCCL, one per process (one process per GPU), created from an
 * id that rank 0 makes and the host distributes by its own means.  gcc_amd's Python host uses torch.distributed (the same
 * RCCL) instead; these entry points serve a host without one.  RCCL is loaded on first use (GCC_ERR_UNSUPPORTED if absent). */
#define GCC_COMM_ID_BYTES 128
typedef struct gcc_comm gcc_comm_t;
int gcc_comm_unique_id(void* id /* [GCC_COMM_ID_BYTES], host */);
int gcc_comm_init(gcc_comm_t** comm, int rank, int world, const void* id);   /* collective; binds to the current device */
/* in-place sum over ranks of count fp32 values, ordered on `stream` like a kernel; the caller applies 1 / world in its
 * optimizer step (gcc_adam_tensor_t.grad_scale) and picks the bucket size (one call per bucket) */
int gcc_comm_allreduce_sum_f32(gcc_comm_t* comm, float* buf, size_t count, gcc_stream_t stream);
/* the same over bf16 values: a gradient bucket cast by gcc_cast_f32_bf16, summed, cast back by gcc_cast_bf16_f32 moves half the
 * bytes over xGMI; every rank receives the same sums, so replicas stay identical.  Both all-reduce entry
 * points are part of a launch recording (gcc_replay_begin) made on the calling thread; a recording that holds one is replayed
 * from one host thread, in the recorded order (collectives of a communicator must be issued in one order on every rank). */
int gcc_comm_allreduce_sum_bf16(gcc_comm_t* comm, void* buf, size_t count, gcc_stream_t stream);
int gcc_cast_f32_bf16(const float* src, void* dst, size_t n, gcc_stream_t stream);      /* src 16-byte, dst 8-byte aligned */
int gcc_cast_bf16_f32(const void* src, float* dst, size_t n, gcc_stream_t stream);
int gcc_comm_rank(const gcc_comm_t* comm);
int gcc_comm_world(const gcc_comm_t* comm);
int gcc_comm_count(const gcc_comm_t* comm);      /* ncclCommCount of the communicator (>= 1), or a negative error code */
int gcc_comm_destroy(gcc_comm_t* comm);
/* RCCL's own message for the calling thread's last failing gcc_comm_* call ("" if none failed): a GCC_ERR_LAUNCH from this
 * group otherwise hides which ncclResult it was */
const char* gcc_comm_last_error(void);

/* CycleGAN's image history (utils/image_pool.py:5-54) on the device: gcc_write_i32 stores n <= 16 ints taken BY VALUE (the
 * host's random draws: two per image, mode 0 pass through / 1 store and pass through / 2 swap with slot, and the slot);
 * gcc_image_pool_query moves the pixels: images / out [N][HW][8] bf16, pool [slots][HW][8], sel device [N][2]. */
int gcc_write_i32(int* dst, const int* values, int n, gcc_stream_t stream);
int gcc_image_pool_query(const void* images, void* out, void* pool, const int* sel, int N, size_t HW, int slots,
                         gcc_stream_t stream);

/* ---- launch replay (gcc_amd/csrc/replay.hip) -------------------------------------------------------------------------
 * The reference leaves the host side of an iteration to PyTorch's eager dispatcher (train.py:128-140 calls
 * model.optimize_parameters() per batch); here an iteration is a few thousand launches of this library, and for the small
 * models the HOST's launch rate is the bound.  gcc_replay_begin starts recording on the calling thread: every launch of
 * the library made by that thread (and its memsets / copies, and gcc_event_record / gcc_stream_wait_event) still executes,
 * and is written down with its argument values.  gcc_replay_end closes the recording; gcc_replay_run issues it again.
 * Contract (as for a captured graph): all pointer arguments stay valid and keep their meaning -- inputs are fed through
 * persistent buffers, the iteration's temporaries live in a pool that nothing else allocates from -- and scalars that change
 * from iteration to iteration are patched: gcc_replay_tag_next(tag) marks the next launch the thread records,
 * gcc_replay_patch overwrites one argument of every launch with that tag (gcc_adam_step's launch takes, in this order,
 * tensors, chunks, chunk_elems, lr, beta1, beta2, eps, bias_correction1, sqrt(bias_correction2): gcc_adam_factors gives
 * the last two for a step).  threads > 1 at gcc_replay_end: gcc_replay_run issues each HIP stream's launches from its own
 * host thread (an event wait is issued only after the record it saw while recording).  Not re-entrant per handle. */
typedef struct gcc_replay gcc_replay_t;
int gcc_replay_begin(gcc_replay_t** out);
int gcc_replay_end(gcc_replay_t* r, int threads);
int gcc_replay_run(gcc_replay_t* r);
int gcc_replay_tag_next(int tag);
int gcc_replay_patch(gcc_replay_t* r, int tag, int arg_index, const void* value, size_t bytes);
long long gcc_replay_info(const gcc_replay_t* r, int what);   /* 0 entries, 1 kernel launches, 2 streams, 3 threads, 4 argument bytes */
int gcc_replay_destroy(gcc_replay_t* r);
/* events of the library (hipEventDisableTiming), recorded / waited for through it so that a recording sees them */
int gcc_event_create(void** event);
int gcc_event_destroy(void* event);
int gcc_event_record(void* event, gcc_stream_t stream);
int gcc_stream_wait_event(gcc_stream_t stream, void* event);
/* out[0] = 1 - beta1^step, out[1] = sqrt(1 - beta2^step) as gcc_adam_step passes them to its kernel */
int gcc_adam_factors(float beta1, float beta2, int step, float* out2);

#ifdef __cplusplus
}
#endif
#endif /* GCC_HIP_H */
