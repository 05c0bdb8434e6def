/* dawn_hip.h -- C ABI of libdawn_hip.so: the MI355X (gfx950) kernels behind DAWN's
 * video-flow-diffusion denoising path.
 *
 * The reference (Hanbo-Cheng/DAWN-pytorch) has no FFI layer on this path: every op is a stock
 * PyTorch call inside Python modules.  Each entry point below therefore cites the reference
 * Python symbol (file:line, abbreviations of SURVEY.md: MT = DM_3/modules/
 * video_flow_diffusion_multiGPU_v0_crema_plus_faceemb_ca_multi_test.py, LA = DM_3/modules/
 * local_attention.py) whose arithmetic it replaces.  The Python host side in
 * dawn-pytorch_amd/ binds these with ctypes.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless noted;
 *  - every launch goes to the caller's hipStream_t (`stream`, passed as void*); nothing allocates,
 *    nothing synchronises; workspaces are caller-provided;
 *  - return 0 on success, non-zero on error (dawn_last_error() gives the text); never throws;
 *  - activations are fp32, channels-last per clip: (F frames, H, W, C) row-major, "row" = one
 *    pixel of one frame; the API tensors x / eps keep the reference layout (3, F, h, w).
 */
#ifndef DAWN_HIP_H
#define DAWN_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The ABI number of this header.  dawn_abi_version() returns the one the library was built from; the Python binding derives every
 * argument type from this file and refuses a library whose number differs. */
#define DAWN_ABI_VERSION 8
const char* dawn_last_error(void);
int dawn_abi_version(void);

/* ---- A1/A2/A4/A12/A13 + every Linear: implicit-GEMM convolution on fp32 MFMA ---------------
 * out[row][n] = bias[n] + sum_{tap,c} P(in[pixel(row)+tap][c]) * W[tap][c][n]  (+ epilogue terms)
 * Replaces nn.Conv3d (1,k,k) per frame (MT:229 Block.proj, MT:417 res_conv, MT:176 Downsample,
 * MT:776 init_conv fea part), nn.ConvTranspose3d (MT:167 Upsample; mode 1) and nn.Linear /
 * 1x1 Conv2d projections (MT:505,512,608,609,662,663) with the PreNorm / GroupNorm-apply that
 * precedes them fused as prologue P and the residual that follows fused as epilogue. */
typedef struct dawn_conv_desc {
    const float* in0; const float* in1; /* NHWC sources; in1 may be NULL; channels = [in0 | in1] */
    int C0, C1, ld0, ld1;               /* channels per source, pixel stride (floats) per source */
    int F, Hi, Wi, Ho, Wo;
    int KH, KW, stride, pad;
    int mode;                           /* 0 = conv, 1 = transposed 4x4/s2/p1 as 4 output phases of 2x2 taps (see `border` at the end) */
    const float* w;                     /* packed [K/4][N][4], k = tap*(C0+C1)+c; mode 1: 4 consecutive phase blocks */
    const float* bias;                  /* N or NULL */
    int N;
    const float* row_mean; const float* row_rstd; /* per INPUT pixel: v=(v-mean)*rstd, or NULL */
    const float* ch_a; const float* ch_b;         /* per input channel: v=v*a[c]+b[c], or NULL */
    int pro_act;                                   /* 0 none, 1 SiLU (applied after the affine) */
    const float* pro_add; int ld_add;              /* added after the activation, or NULL */
    const float* res; int ld_res;                  /* epilogue: out += res[row][n], or NULL */
    const float* tr; int ld_tr;                    /* epilogue: out += silu(tr[row][n]*tr_a[n]+tr_b[n]) */
    const float* tr_a; const float* tr_b;
    float* out; int ld_out;
    double* gn_part;                               /* optional: per-block GroupNorm(8) partial sums of the output,
                                                      [gridDim.x][16] = (sum, sumsq) per group (see dawn_gn_reduce) */
    const void* w_bf3;                             /* optional (3x3/s1/p1 convs, large 1x1 GEMMs): the same weights split exactly into three
                                                      bf16 planes w = w1+w2+w3, [K/16][3][2][N][8] (k = tap*(C0+C1)+c), for
                                                      the split-operand bf16-MFMA kernel; NULL = fp32 MFMA */
    int* gn_rows;                                  /* optional HOST pointer: receives the number of gn_part rows this launch
                                                      writes (<= dawn_conv_gemm_nblocks); negative = the launch also finalised (gn_a below) */
    int policy;                                    /* kernel-selection bits (DAWN_POLICY_* below); 0 = shipped default */
    float ln_eps;                                  /* > 0: LayerNorm (no gain) over the C0+C1 channels of every input row, computed by the
                                                      GEMM itself -- no statistics pass (instead of row_mean / row_rstd).  <= 128 channels: from the
                                                      rows it holds in registers; deeper narrow projections: one shifted one-pass statistics sweep
                                                      per row panel before its K loop.  Only shapes with dawn_gemm1x1_ln_inline_ok, error otherwise */
    void* sk_ws; size_t sk_ws_bytes;               /* RESERVED, leave NULL / 0 (kept for the struct layout).  Round 3: hand-off scratch of a persistent stream-K
                                                      form of the 3x3 kernel -- faster in isolation, slower end to end on a power-limited chip; since round 4 that
                                                      kernel lives in tools/ubench/conv3x3_sk.hip and exists only in the experimental library of
                                                      the hipbuild.py sktiming preset.  The shipped library ignores both fields */
    const void* w_wino;                            /* optional (3x3/s1/p1 convs): the Winograd F(2x2,3x3) image of the weights, U = G g G^T computed in
                                                      fp64 and split into three bf16 planes, in the fragment order of conv3x3_wino_kernel:
                                                      [(C0+C1)/16][16 positions][N/16][2][64 lanes][8] (pack.pack_wino_bf3).  With
                                                      DAWN_POLICY_WINO2 such convs run in the Winograd form (2.25x fewer matrix-pipe flops, fp32 results to
                                                      fp32-Winograd accuracy); NULL or other shapes = the direct split kernel */
    /* optional, with gn_part: finish the GroupNorm in the conv launch itself (dawn_gn_reduce_finalize's arguments: MT:230-248) -- the
     * workgroup that finishes last reduces the partial rows in fixed order and writes a[c] / b[c].  Honoured by the Winograd kernel
     * only; *gn_rows < 0 then says so (|*gn_rows| rows were written), otherwise call dawn_gn_reduce_finalize as before.  gn_ticket =
     * one device word per stream.  HARD PRECONDITION: it is ZERO when the launch starts (dawn_gn_ticket_reset; a completed launch
     * leaves it zero).  With a non-zero ticket (an aborted launch, an uninitialised word) no workgroup sees itself as the last one:
     * gn_a / gn_b are then NOT written although *gn_rows reports them -- so reset it at the start of every evaluation, as both hosts
     * do.  ISA-level assumption of the hand-off (conv3x3_wino.hip): the gn_part rows and the ticket are agent-scope RELAXED atomics
     * (write-through to / read from the device-coherent level), ordered by `s_waitcnt vmcnt(0)` + a workgroup barrier before the
     * ticket's read-modify-write; the last workgroup's row loads are agent-scope atomic loads issued after its own RMW returned.
     * No release/acquire fence: on gfx950 a release writes back the XCD's whole L2 (measured -4.5 % on the benchmark). */
    const float* gn_gamma; const float* gn_beta; const float* gn_fs; const float* gn_fsh;
    double gn_count; float gn_eps;
    float* gn_a; float* gn_b;
    unsigned* gn_ticket;
    /* round 5 (ABI 7), optional: the Winograd F(4x4,3x3) image of a 3x3 / stride-1 / pad-1 conv (pack.pack_wino4_bf3: [(C0+C1)/16][36
     * positions][N/16][768 bf16 = the fragment [u1|u2] in lane order, then u3 of the k-groups 0, 1] of U = G g G^T on the points 0, +-3/4,
     * +-3/2, inf: every plane once, 8 of the 9 cross terms).  With DAWN_POLICY_WINO4 (in the shipped default: the form only for
     * the shapes it measured faster on; DAWN_POLICY_WINO4_ALL_SHAPES adds every shape dawn_conv3x3_wino4_ok accepts) the conv runs as conv3x3_wino4_kernel (4x fewer
     * matrix-pipe flops than the direct form, fp32 results to fp32-F(4x4) accuracy: ~2x the direct form's rounding error); the gn_* fields
     * above are honoured exactly as by the F(2x2) kernel */
    const void* w_wino4;
    /* mode 1 only: what a 2x2 phase tap outside the Hi x Wi input reads.  0 = zero (the transposed conv; what a zero-initialised
     * descriptor says), 1 = the edge pixel (index clamped), 2 = the opposite edge (index wrapped).  With the folded weights of
     * pack.upconv_w_kn_phases this is nn.Upsample(scale (1,2,2), nearest) + nn.Conv3d (1,3,3)/s1/p(0,1,1) of MT:169-172 without the
     * upsampled tensor: padding_mode zeros = 0, reflect and replicate = 1 (the padded row of the upsampled image is a copy of the
     * edge row either way), circular = 2.  Pixels whose four taps are in range take the same path for every value.  Non-zero in
     * mode 0, or any other value: error -15, nothing is launched. */
    int border;
} dawn_conv_desc;
int dawn_conv_gemm(const dawn_conv_desc* d, void* stream);
/* 1 when a 3x3 / stride 1 / pad 1 conv of this shape (F frames of H x W pixels, C0 + C1 input channels, N output channels) runs in the
 * Winograd F(2x2,3x3) form once dawn_conv_desc.w_wino is supplied (DAWN_POLICY_WINO2, in the shipped default): image width a power
 * of two <= 64, even height, 256-pixel tiles, an even number of 16-channel chunks, N a multiple of 64 */
int dawn_conv3x3_wino_ok(int F, int H, int W, int C0, int C1, int N);
/* the same question for the F(4x4,3x3) form (dawn_conv_desc.w_wino4, DAWN_POLICY_WINO4): image width 64 or 32, H a multiple of
 * 256 / W, an even number of 16-channel chunks, N a multiple of 64 */
int dawn_conv3x3_wino4_ok(int F, int H, int W, int C0, int C1, int N);
/* Which form of the 3x3 conv dawn_conv_gemm would run for this descriptor (host code, launches nothing; the launch's own decision
 * code): 2 = Winograd F(4x4,3x3), 1 = Winograd F(2x2,3x3), 0 = anything else. */
int dawn_conv3x3_form(const dawn_conv_desc* d);
/* Which DIRECT split-operand 3x3 kernel dawn_conv_gemm would run for this descriptor (host code, launches nothing; the launch's own
 * decision code, tile width included -- it depends on the number of rows, so fewer frames can land on another kernel): */
#define DAWN_DIRECT3X3_NONE 0     /* none: a Winograd form or a split 1x1 / resample kernel takes it, or it falls to the fp32 kernels */
#define DAWN_DIRECT3X3_HALO 1     /* conv3x3_halo_bf16_kernel (v1) */
#define DAWN_DIRECT3X3_V2_WN1 2   /* conv3x3_bf16_v2_kernel, 256 x 64 tiles (four waves) */
#define DAWN_DIRECT3X3_V2_WN2 3   /* conv3x3_bf16_v2_kernel, 256 x 128 tiles (eight waves) */
int dawn_conv3x3_direct_form(const dawn_conv_desc* d);
/* Which split-operand kernel dawn_conv_gemm would run a 1x1 projection or a 4x4 / stride-2 resample descriptor on (host code, launches
 * nothing; the launch's own decision code): */
#define DAWN_SPLIT1X1_NONE 0      /* none of them: the 3x3 paths or the fp32 kernels */
#define DAWN_SPLIT1X1_TILED 1     /* gemm1x1_bf16_kernel (256 x 64 / 256 x 128 / 128 x 64 tiles) */
#define DAWN_SPLIT1X1_ROWREG 2    /* gemm1x1_rowreg_kernel (K = 64 / 128, rows stationary in registers) */
#define DAWN_SPLIT1X1_ROWACC 3    /* gemm1x1_rowacc_kernel (K >= 256, N <= 192) */
#define DAWN_SPLIT1X1_RESAMPLE 4  /* gemm1x1_rowacc_kernel in its Downsample (4x4 / stride 2) or Upsample (2x2 phases) mode */
int dawn_gemm1x1_form(const dawn_conv_desc* d);
/* upper bound on the thread blocks (= rows of gn_part) dawn_conv_gemm launches for an (M rows, N columns) output;
 * the launch reports the exact count through dawn_conv_desc.gn_rows */
int dawn_conv_gemm_nblocks(long M, int N);
/* ---- dawn_conv_desc.policy: THE table of its bits (0 = DAWN_CONV_POLICY_DEFAULT; per call, no process-global state; read through policy_of() of
 * csrc/conv_split.h, which drops what the build does not honour; measurement history longer than a line: DESIGN.md).  Status: shipped = in the default;
 * A/B = honoured by the shipped library, measured, not in the default (every such combination computes the same function: the tests run the kernel families
 * against each other); ablation = -DDAWN_ABLATION builds only (hipbuild.py presets; wrong results by design); sktiming = the experimental stream-K build only. */
#define DAWN_POLICY_BK32               0x1         /* fp32 kernel: BK = 32 tiles for deep-K GEMMs (K >= 4096, N > 64).  shipped (profiles/r1_d_conv_variants.txt) */
#define DAWN_POLICY_TILE256            0x2         /* fp32 kernel: 256 x 64 tiles for N <= 64.  A/B: no gain (profiles/r1_d_conv_variants.txt) */
#define DAWN_POLICY_XCD_ORDER          0x4         /* XCD-contiguous tile order for multi-tap convs on >= 32 x 32 frames.  shipped (profiles/r1_d_conv_variants.txt) */
#define DAWN_POLICY_GLDS               0x8         /* direct-to-LDS staging for prologue-free fp32 GEMMs.  shipped (profiles/r1_j_conv_glds.txt) */
#define DAWN_POLICY_ABL_NO_RESTAGE     0x10        /* fp32 kernel without re-staging.  ablation */
#define DAWN_POLICY_ABL_NO_BARRIER     0x20        /* ... and without its barrier.  ablation */
#define DAWN_POLICY_SK_PRIO_ALT        0x40        /* stream-K kernel: issue-priority alternation (period in DAWN_POLICY_VARIANT).  sktiming; ignored by the shipped library */
#define DAWN_POLICY_GLDS_BK32          0x80        /* direct-to-LDS path: BK = 32 for every shape.  A/B */
#define DAWN_POLICY_GLDS_STAGES3       0x100       /* direct-to-LDS path: 3-stage counted-vmcnt pipeline.  A/B: no gain (profiles/r1_j_conv_glds.txt) */
#define DAWN_POLICY_GLDS_TILE256       0x200       /* direct-to-LDS path: its 256 x 64 tile for every N <= 64 GEMM of >= 65536 rows.  A/B */
#define DAWN_POLICY_SK_NO_PAIR_OFFSET  0x200       /* (same bit) stream-K kernel: no half-tile offset between co-resident workgroups.  sktiming */
#define DAWN_POLICY_GLDS_NO_TILE256    0x400       /* direct-to-LDS path: never that tile (automatic for 3x3 convs of <= 64 channels).  A/B */
#define DAWN_POLICY_STREAMK            0x400       /* (same bit) the persistent stream-K 3x3 kernel where sk_ws is supplied.  sktiming (profiles/r3_conv_sk_vs_v2_in_benchmark.txt) */
#define DAWN_POLICY_HALO               0x800       /* LDS-halo fp32 kernel for prologue-free 3x3 / s1 / p1 convs.  shipped (profiles/r1_l_conv_halo.txt) */
#define DAWN_POLICY_SPLIT              0x1000      /* split-operand (bf16 pipe) kernels where w_bf3 is supplied.  shipped (profiles/r1_n_conv_bf16.txt) */
#define DAWN_POLICY_NINE_TERMS         0x2000      /* all 9 cross terms instead of 6, direct kernels only (no Winograd form).  A/B: the accuracy yardstick of the tests */
#define DAWN_POLICY_SPLIT_V2           0x4000      /* second-generation split 3x3 kernel (conv3x3_bf16_v2_kernel).  shipped (profiles/r1_n_conv_bf16.txt) */
#define DAWN_POLICY_TILE128_ALWAYS     0x8000      /* tiled split 1x1 GEMM: 128 x 64 tiles for every eligible shape.  A/B (profiles/r2_gemm1x1_tiles_128x64.txt) */
#define DAWN_POLICY_TILE128_NEVER      0x10000     /* tiled split 1x1 GEMM: never 128 x 64 tiles (the round-1 tile policy).  A/B (profiles/r2_gemm1x1_tiles_128x64.txt) */
#define DAWN_POLICY_NO_ROW_KERNELS     0x20000     /* the tiled kernel for every split 1x1 shape: no row-stationary / resample kernels.  A/B */
#define DAWN_POLICY_XCD_LAUNCH_ORDER   0x80000     /* tiled split 1x1 GEMM: tiles dealt to the XCDs in launch order.  A/B; read RAW (policy_raw_bit): outside both masks */
#define DAWN_POLICY_VARIANT(n)         ((n) << 16) /* field, shift 16 width 4.  ablation: build n of the split 3x3 kernel (1, 2, 4, 7 ablated, 8 = s_memtime stamps); sktiming: priority period */
#define DAWN_POLICY_VARIANT_MASK       0xF0000     /* OVERLAP, only under -DDAWN_ABLATION: its values 1, 2, 8 ARE TILE128_NEVER, NO_ROW_KERNELS, XCD_LAUNCH_ORDER; the shipped mask keeps the first two, drops the rest */
#define DAWN_POLICY_STAGGER(n)         ((n) << 20) /* field, shift 20 width 4: start delay of workgroup sets (split v2, Winograd; sktiming: slots left free).  A/B (profiles/r5_wino4_stagger.txt); DROPPED by the -DDAWN_ABLATION mask although both Winograd units read it */
#define DAWN_POLICY_STAGGER_MASK       0xF00000    /* the bits of that field */
#define DAWN_POLICY_MFMA_K32           0x1000000   /* split v2 kernel on v_mfma_f32_16x16x32_bf16 (two cross terms per instruction).  shipped (profiles/r3_k32_shapes.txt) */
#define DAWN_POLICY_WINO2              0x2000000   /* Winograd F(2x2,3x3) form where w_wino is supplied and dawn_conv3x3_wino_ok.  shipped (profiles/r4_wino_insitu_per_shape.txt) */
#define DAWN_POLICY_WINO2_DEEP_ONLY    0x4000000   /* ... but the direct kernel for convs of fewer than 128 input channels.  A/B: slower (profiles/r5_ab_gn_sums_and_per_shape_policy.txt) */
#define DAWN_POLICY_WINO4              0x8000000   /* Winograd F(4x4,3x3) form where w_wino4 is supplied, dawn_conv3x3_wino4_ok and the shape measured faster (64 channels at width 64, <= 128 at width 32).  shipped (profiles/r5_ab_wino4_policy_in_benchmark.txt) */
#define DAWN_POLICY_WINO4_ALL_SHAPES   0x10000000  /* with WINO4: wherever the form fits.  A/B (profiles/r5_insitu_shapes_wino4_everywhere_vs_gated.txt) */
#define DAWN_POLICY_WINO_REVERSE       0x20000000  /* both Winograd kernels walk their tiles last frame first (bit-identical outputs).  shipped (profiles/r5_ab_wino_reverse_order.txt) */
#define DAWN_POLICY_ABL_ROW_FETCH      0x40000000  /* row-stationary GEMMs fetch rows line-coalesced into the wrong lanes.  ablation (profiles/r5_row_fetch_pattern_ablation.txt); read RAW (policy_raw_bit): outside both masks */
#define DAWN_CONV_POLICY_DEFAULT /* = 0x2B00580D */ (DAWN_POLICY_BK32 | DAWN_POLICY_XCD_ORDER | DAWN_POLICY_GLDS | DAWN_POLICY_HALO | DAWN_POLICY_SPLIT | \
                                  DAWN_POLICY_SPLIT_V2 | DAWN_POLICY_MFMA_K32 | DAWN_POLICY_WINO2 | DAWN_POLICY_WINO4 | DAWN_POLICY_WINO_REVERSE)

/* ---- A3 GroupNorm(8) statistics over (C/8, F, H, W) (MT:230,235; nn.GroupNorm on a 5-D tensor) --
 * partial: per-block fp64 (sum, sumsq) per group -> part[nblk][16]; reduce: fixed-order sum ->
 * sums[16] (all-reduced across T-shards by the caller); finalize: per-channel fused coefficients
 *   a[c] = rstd*gamma*(fs+1), b[c] = (beta-mean*rstd*gamma)*(fs+1)+fsh   (FiLM fs/fsh optional, MT:237-239) */
int dawn_gn_partial(const float* x, long rows, int C, int ld, double* part, int nblk, void* stream);
int dawn_gn_reduce(const double* part, int nblk, double* sums16, void* stream);
int dawn_gn_finalize(const double* sums16, double count_per_group, const float* gamma, const float* beta,
                     const float* film_scale, const float* film_shift, int C, float eps,
                     float* a, float* b, void* stream);
/* reduce + finalize in one launch (single-GPU path: no all-reduce between them) */
int dawn_gn_reduce_finalize(const double* part, int nblk, double count_per_group, const float* gamma,
                            const float* beta, const float* film_scale, const float* film_shift, int C,
                            float eps, float* a, float* b, void* stream);
/* zero the hand-off word(s) of the fused GroupNorm finalisation (dawn_conv_desc.gn_ticket; 16 bytes): stream-ordered fill, once per
 * evaluation before its first conv launch (graph-capturable) */
int dawn_gn_ticket_reset(unsigned* ticket, void* stream);
/* out = silu(x*a[c]+b[c]) + res   (Block.act MT:248 + residual add MT:479); out may be x itself (in place) */
int dawn_gn_apply_res(const float* x, const float* a, const float* b, const float* res, float* out,
                      long rows, int C, void* stream);

/* ---- PreNorm LayerNorm / LayerNorm_img statistics per pixel over [in0|in1] channels (MT:179-203) */
int dawn_ln_rowstats(const float* in0, int C0, int ld0, const float* in1, int C1, int ld1, long rows,
                     float eps, float* mean, float* rstd, void* stream);
/* same statistics, but writes the normalised rows xn (rows, C0+C1) = (x - mean) * rstd, so that the consuming
 * projection (gain folded into its weights) runs as a prologue-free direct-to-LDS GEMM */
int dawn_ln_rows(const float* in0, int C0, int ld0, const float* in1, int C1, int ld1, long rows, float eps,
                 float* xn, void* stream);

/* ---- A5 tri-modal CrossAttention (MT:516-559) ------------------------------------------------
 * prep (once per clip): kv (F,128) from to_kv -> kvtab[f][branch] = [l2norm(k_h)*k_scale | v]  */
int dawn_xattn_prep(const float* kv, int F, const float* k_scale, const float* null_kv,
                    float* kvtab, int branch, float* nulltab, void* stream);
/* core: q (rows,192)=[branch][head][8] -> o (rows,192): 2-key cosine-sim softmax == sigmoid lerp */
int dawn_xattn_core(const float* q, float* o, long rows, int HW, const float* kvtab, const float* nulltab,
                    const float* q_scale, void* stream);
/* h_cond[row][c] = sum_b LayerNorm_img(y3[row][b][:])[c] * g[b][c]   (to_out.1, MT:513; sum MT:463) */
int dawn_xattn_ln_sum(const float* y3, const float* g3, float* out, long rows, int Co, float eps, void* stream);

/* Per-clip tables of one conditioned block (the condition is DDIM-step-invariant, so this runs once per clip):
 * xtab (F,3,64+9*Co): per (frame, branch)  D[h][i] = q_scale[i] (k_null[i] - k_ctx[h][i]) 8 log2(e)   (64 floats),
 * u_h = Wo[8h..8h+7]^T (v_ctx,h - v_null) for h = 0..7 and y0 = Wo^T v_null (9 rows of Co).  With them the 2-key
 * softmax is sigma_h = 1 / (1 + 2^(q_h . D_h / |q_h|)) and to_out(o) = y0 + sum_h sigma_h u_h  (exact rewrites of
 * MT:540-558).  kvtab / nulltab from dawn_xattn_prep; wo0..2 packed (64 -> Co). */
int dawn_xattn_tables(const float* kvtab, const float* nulltab, const float* q_scale, const float* wo0,
                      const float* wo1, const float* wo2, int F, int Co, float* xtab, void* stream);
/* Levels without the fused kernel (Co = 128 / 256 / 512; any Co % 32 == 0 up to 512, H*W % 4 == 0): everything after the
 * Q projection in one pass -- q (rows,192) raw to_q output, xtab (F,3,64+9*Co) from dawn_xattn_tables, g3 (3,Co):
 * out[row][:] = sum_b LN(y0_b + sum_h sigma_bh u_bh) * g3[b]   ==   dawn_xattn_core + 3 x to_out + dawn_xattn_ln_sum. */
int dawn_xattn_sigma_out_h1(const float* q, long rows, int HW, const float* xtab, const float* g3, int Co, float eps,
                            const float* gn_x, const float* gn_a, const float* gn_b, float* out, void* stream);   /* same, gn_x (rows, Co) */
int dawn_xattn_sigma_out(const float* q, long rows, int HW, const float* xtab, const float* g3, int Co, float eps,
                         float* out, void* stream);
/* Fused cross-attention branch for Co = 64, Cin in {64, 128} (two sources allowed), H*W % 32 == 0:
 * out[row][:] = sum_b LN(to_out_b(attn_b(LN([in0|in1][row]))))  -- everything of MT:454-468 / MT:516-559 in one launch.
 * wq packed (Cin -> 192, LayerNorm gains folded), g3 (3,64), xtab (F,3,640) from dawn_xattn_tables.
 * wq_bf3 (optional): the exact 3-way bf16 split of wq, [Cin/16][3][2][192][8] (pack_bf3 order): to_q then runs on the bf16
 * matrix pipe (fp32 results, 6 cross terms); NULL = fp32-MFMA projection. */
/* ... and the block's h1 = SiLU(FiLM(GroupNorm(c1))) + h_cond (MT:473-476) written straight from the epilogue: gn_x = c1 (rows, 64),
 * (gn_a, gn_b) = the per-channel coefficients of dawn_gn_finalize -- no h_cond tensor and no dawn_gn_apply_res pass (NULL: h_cond).
 * `out` MAY BE `gn_x` (here and in dawn_xattn_sigma_out_h1): the epilogue reads an element of c1 and writes the same element of h1. */
int dawn_xattn_layer_c64_h1(const float* in0, int C0, int ld0, const float* in1, int C1, int ld1, long rows, int HW,
                            const float* wq, const void* wq_bf3, const float* g3, const float* xtab, float eps, const float* gn_x,
                            const float* gn_a, const float* gn_b, float* out, void* stream);
int dawn_xattn_layer_c64(const float* in0, int C0, int ld0, const float* in1, int C1, int ld1, long rows, int HW,
                         const float* wq, const void* wq_bf3, const float* g3, const float* xtab, float eps, float* out,
                         void* stream);

/* ---- A9/A10 windowed temporal self-attention per pixel (MT:665-725 with the MT:117 window mask,
 * == LA:71-99/300-342).  qkv (Fext*HW, 768) = [q|k|v][head 8][32]; queries are frames
 * [q0, q0+Fq) of the buffer, keys every buffer frame within +-win; rotary (interleaved pairs)
 * from cos/sin tables (Fext,16); band[(2*win+1)][8] = relative-position bias by offset j-i. */
int dawn_temporal_attn(const float* qkv, int Fext, int HW, int q0, int Fq, int win,
                       const float* rot_cos, const float* rot_sin, const float* band,
                       float* out, void* stream);
/* the same with flags: 0 = automatic (S and P.V on the bf16 matrix pipe with exactly split operands where the shape is covered:
 * win <= 48, at most 256 queries, K / V planes of the buffer in LDS, >= 128 pixel columns; the fp32-MFMA kernel otherwise) */
#define DAWN_TA_FP32          1   /* the fp32-MFMA kernel even where the split-operand kernel covers the shape.  A/B, tests */
#define DAWN_TA_SPLIT_ALWAYS  2   /* the split-operand 32 x 32 kernel whatever the number of pixel columns.  A/B, tests */
#define DAWN_TA_WAVE13        4   /* the window-tiled 13-wave kernel (16-query tiles, temporal_attn13_kernel; win <= 40, Fext <= 208, at most 13 query
                                     tiles: error -39 outside).  A/B: +4..9 % isolated, -0.3 % in the benchmark (profiles/r6_temporal_attn13_ab.txt) */
#define DAWN_TA_PIXEL_HEAD_MAJOR 16  /* with WAVE13 only: qkv is [pixel][head][q | k | v][buffer row][32] (the layout experiment of DESIGN 8).  A/B */
int dawn_temporal_attn_ex(const float* qkv, int Fext, int HW, int q0, int Fq, int win,
                          const float* rot_cos, const float* rot_sin, const float* band,
                          float* out, int flags, void* stream);

/* Fused LAYER for 64-channel levels: out[(i-q0)] = x[i] + to_out(attn(LayerNorm(x)))  (MT:179-188, 665-725,
 * 141-147) -- x (Fext*HW, 64) rows, packed wqkv [(64/4)][768][4] (LayerNorm gain folded), wout [(256/4)][64][4].
 * Limits: Fext <= 288, Fq <= 256, win <= 48; the caller falls back to the unfused ops otherwise.
 * wqkv_bf3 (optional): exact 3-way bf16 split of wqkv, [64/16][3][2][768][8] (pack_bf3 order): when the LDS budget
 * allows (Fext <= 224) the Q/K/V projections run on the bf16 matrix pipe with fp32 results; NULL = fp32 MFMA. */
int dawn_temporal_layer_c64(const float* x, int Fext, int HW, int q0, int Fq, int win, const float* wqkv,
                            const void* wqkv_bf3, const float* wout, const float* rot_cos, const float* rot_sin,
                            const float* band, float eps, float* out, void* stream);
/* same, with a kernel-family selector for A/B measurements and tests (DAWN_TL_* below): force field 0 = automatic (what the entry
 * point above does), DAWN_TL_FORCE_WMODE(m) forces WMODE m: 0 fp32 MFMA with weights from L2, 1 fp32 MFMA with per-head weight slices in LDS, 2 Q/K/V
 * projections on the bf16 pipe (exact 3-way operand split), 3 additionally S = K.Q^T and O = V^T.P^T on the bf16 pipe
 * (K / V split once per head into bf16 planes in LDS, Q / P split from the accumulators; fits up to Fext ~ 200 rows:
 * the benchmark clip).  wout_bf3p (optional, WMODE 3): the exact
 * 3-way bf16 split of to_out with the rows of every head permuted to the accumulator order of O^T, [256/16][3][2][64][8]
 * (pack.pack_bf3_temporal_out).  All families compute the same function to fp32 round-off.
 * `out` MAY BE `x` when the layer covers its whole frame buffer (q0 == 0, Fq == Fext): a workgroup reads the rows of its pixel
 * before it writes them and no other workgroup touches them (the denoiser's unsharded 64-channel layers run that way:
 * one tensor less through the caches).
 * Round 6 (ABI 8): WMODE 4 = the WINDOW-tiled kernel (csrc/temporal_layer16.hip): 16-query tiles against the 16 + 2 win <= 96 keys
 * of their window (only the key blocks that exist at the clip ends) on v_mfma_f32_16x16x32_bf16, 12 waves, the head's work split
 * into two SIMD-balanced phases by dawn_tl16_schedule.  Automatic whenever both split weight images are given,
 * win <= 40 and Fext <= 208; forced: error if the shape is outside; DAWN_TL_KEEP_32X32 keeps the 32 x 32 kernel.
 * WMODE 5 = the same window tiling with ONE query tile per wave (13 waves of 128 registers instead of 8 of 256: no wave runs two tiles one
 * after the other): taken first by the automatic choice whenever the query range has at most 13 tiles (208 - delta frames). */
#define DAWN_TL_FORCE_MASK     7            /* the force field: 0 = automatic */
#define DAWN_TL_FORCE_WMODE(m) ((m) + 1)    /* its value that forces WMODE m (0..5); error -36 / -37 / -38 where WMODE 3 / 4 / 5 does not cover the shape */
#define DAWN_TL_SCHED_HINTS    16           /* WMODE 3 with explicit sched_group_barrier MFMA / VALU interleave hints.  A/B: within noise (1550 vs 1513 us) */
#define DAWN_TL_OUT_FP32       32           /* WMODE 3 keeps its out-projection on the fp32 MFMA even when wout_bf3p is given.  A/B, tests */
#define DAWN_TL_NO_FIXED200    64           /* WMODE 3 without the fixed 200-row LDS layout of clips of <= 200 buffer rows.  A/B, tests */
#define DAWN_TL_NO_KVI         128          /* WMODE 3 projects K / V one wave per 32-row tile, not as 2 nrt (tile, K | V) items dealt over the waves (KVI).  A/B, tests */
#define DAWN_TL_KEEP_32X32     256          /* automatic choice without the window-tiled kernels (WMODE 4 / 5).  A/B, tests */
int dawn_temporal_layer_c64_ex(const float* x, int Fext, int HW, int q0, int Fq, int win, const float* wqkv,
                               const void* wqkv_bf3, const float* wout, const void* wout_bf3p, const float* rot_cos,
                               const float* rot_sin, const float* band, float eps, float* out, int flags, void* stream);

/* The work split of the window-tiled layer (host code, no GPU): per wave of the 12-wave workgroup one word --
 * bits 0..4 / 5..9 its query tiles (31 = none), 10..12 its K / V projection group (0 K features 0..15, 1 K 16..31, 2 / 3 V; 7 = none),
 * 13..17 / 18..22 the group's 16-row tiles [t0, t1).  Waves w, w + 4, w + 8 share a SIMD; simd_units (optional, 8 ints) receives the
 * MFMA count per SIMD and head of phase A (projections) and phase B (attention).  Returns 0 when the shape is outside the kernel. */
typedef struct dawn_tl16_sched { unsigned w[12]; } dawn_tl16_sched;
int dawn_tl16_schedule(int Fext, int q0, int Fq, int win, dawn_tl16_sched* sched, int* simd_units);
/* The work split of the 13-wave form (WMODE 5; host code, no GPU): 16 words, one per wave slot (13 used) -- bits 0..4 the wave's ONE query
 * tile (31 = none), 5..7 its K / V projection group (as above; 7 = none), 8..12 / 13..17 the group's 16-row tiles [t0, t1).  Wave w runs on
 * SIMD w & 3 (SIMD 0 holds four waves, the others three): the tiles are dealt so that the per-SIMD sums of the tile costs balance, the row
 * tiles of a group evenly over the waves of its SIMD.  Returns 0 when the shape is outside the kernel (more than 13 query tiles, win > 40,
 * more than 208 rows). */
int dawn_tl13_schedule(int Fext, int q0, int Fq, int win, unsigned* words16);

/* ---- A8 SpatialLinearAttention core (MT:611-627) ---------------------------------------------- */
int dawn_sla_context(const float* qkv, int F, int HW, float* ctx, void* stream);     /* ctx (F,8,32,32) */
int dawn_sla_apply(const float* qkv, const float* ctx, int F, int HW, float* out, void* stream); /* out (F*HW,256) */

/* Fused LAYER for 64-channel levels: out = x + to_out(linattn(LayerNorm(x))) + bias, q/k/v never materialised.
 * M_ws: caller workspace of dawn_sla_ws_floats(F, HW, wqkv_bf3 != NULL) floats (per-frame folded context . to_out matrices
 * and, on the split-operand path, the per-slice partial contexts of the sliced sweep).
 * wqkv_bf3 (optional): the exact 3-way bf16 split of wqkv, [64/16][3][2][768][8] (pack_bf3 order): the context
 * kernel then runs its K / V projections on the bf16 matrix pipe (fp32 results) in a single sweep with a running
 * column max, sliced over the frame's pixels so that every CU works (partials merged by a small second kernel), and the
 * apply kernel runs its Q projection there; NULL = two-sweep fp32-MFMA kernels.  `out` MAY BE `x`: the context kernel(s) have read
 * every row before the apply kernel starts, and an apply workgroup reads its own rows before it writes them. */
long dawn_sla_ws_floats(int F, int HW, int split);
int dawn_sla_layer_c64(const float* x, int F, int HW, const float* wqkv, const void* wqkv_bf3, const float* wout,
                       const float* bias, float eps, float* M_ws, float* out, void* stream);

/* ---- A11 mid spatial attention: full softmax attention over the HW tokens of a frame (MT:841-843) */
int dawn_frame_attn(const float* qkv, int F, int N, float* out, void* stream);

/* ---- A1 x-part of init_conv (3 of 275 channels) + hoisted fea part + bias (MT:776-777, 910) ------
 * x (3,F,h,w) reference layout; w3 [7*7*3][Co] ; fea_pre (h,w,Co) = conv7x7(fea272)+bias; out (F,h,w,Co) */
/* the same on a frame sub-range of a longer latent: x points at its first frame, plane_stride = floats between channel planes */
int dawn_init_conv_x_ex(const float* x, long plane_stride, const float* w3, const float* fea_pre, int F, int h, int w, int Co,
                        float* out, void* stream);
int dawn_init_conv_x(const float* x, const float* w3, const float* fea_pre, int F, int h, int w, int Co,
                     float* out, void* stream);
/* ---- A13 heads: two 1x1 convs (Co->2, Co->1) + concat, written as (3,F,h,w) (MT:863,876,956); hg or ho may be NULL: only the
 * other head's rows of eps_out are written ------ */
int dawn_head_out(const float* hg, const float* ho, const float* wg, const float* bg, const float* wo,
                  const float* bo, long rows, int Co, float* eps_out, void* stream);
/* ---- the same heads with each head block's res_conv (MT:417) folded into its output projection: one streaming kernel from the
 * blocks' conv2 outputs to eps, eps[0:2] = Wg.SiLU(a2g*c2g + b2g) + Wf[0:2].[in0|in1] + bf[0:2], eps[2] = Wo.SiLU(a2o*c2o + b2o) +
 * Wf[2].[in0|in1] + bf[2] (a2 / b2: the GroupNorm coefficients of dawn_gn_finalize, length Co; Wf (3, C0 + C1) and bf (3) from
 * dawn_fold_heads, on the device).  c2g or c2o (with its a / b) may be NULL: only the other head's rows of eps_out (3, rows) are
 * written.  Co, C0, C1, ld0, ld1 multiples of 4, at most 256 channels per source, 16-byte aligned pointers: anything else is
 * refused with an error code (the caller then runs res_conv through dawn_conv_gemm and dawn_head_out) */
int dawn_heads_eps(const float* c2g, const float* a2g, const float* b2g, const float* c2o, const float* a2o, const float* b2o,
                   const float* in0, int ld0, int C0, const float* in1, int ld1, int C1, const float* wg, const float* wo,
                   const float* Wf, const float* bf, long rows, int Co, float* eps_out, void* stream);
/* host only (every pointer is host memory): Wf[0:2] = Wg.Wr_g, Wf[2] = Wo.Wr_o, bf = [Wg.br_g + bg ; Wo.br_o + bo] with wg (2, Co),
 * wo (1, Co), wr_g / wr_o (Co, Cin) row-major (the res_conv weights as the checkpoint holds them); summed over co in ascending order
 * in fp64 and rounded to fp32 once.  A constant of the model: computed once per packed model */
int dawn_fold_heads(const float* wg, const float* bg, const float* wo, const float* bo, const float* wr_g, const float* br_g,
                    const float* wr_o, const float* br_o, int Co, int Cin, float* Wf, float* bf);

/* ---- small dense ops: time / condition MLPs (MT:366-384, 789-794) ----------------------------- */
/* out[m][n] = bias[n] + sum_k act(in[m][k]) * W[n][k];  act_in: 0 none, 1 SiLU, 2 exact GELU */
int dawn_linear(const float* in, int M, int K, int ld_in, const float* W, const float* bias, int N,
                int act_in, float* out, int ld_out, void* stream);
/* SinusoidalPosEmb MT:150-162; freqs (dim/2) = exp(-i*ln(1e4)/(dim/2-1)) table computed once on the host */
int dawn_sinusoidal(float t, int dim, const float* freqs, float* out, void* stream);

/* ---- A0 DDIM sampler step pieces (MT:1169-1205) ------------------------------------------------ */
/* x0 = recip*x - recipm1*eps ; also histogram of the top 11 bits of |x0| into hist[2048] */
int dawn_ddim_x0(const float* x, const float* eps, float recip, float recipm1, long n, float* x0,
                 unsigned* hist, void* stream);
/* radix-select helpers for the exact q-quantile of |x0| (torch.quantile, linear interpolation): `rank` / `weight` = floor and fraction
 * of q * (n - 1), any q in [0, 1] (q = 1: rank n - 1, no element above it, the result is the maximum; q = 0: rank 0, weight 0) */
int dawn_select_scan(const unsigned* hist, int nbins, unsigned long long rank, unsigned* state, int pass,
                     void* stream);
int dawn_select_hist(const float* x0, long n, const unsigned* state, int pass, unsigned* hist, void* stream);
int dawn_select_finalize(const unsigned* state, const unsigned* hist3, float weight, float* s_out, void* stream);
/* scratch of one selection [hist1 2048 | hist2 1024 | hist3 1024 | state 4 | hmin 4] = 4104 words: zero histograms and state,
 * hmin = INT_MAX (two stream-ordered fills; the host reuses one buffer per device for every DDIM step) */
int dawn_select_ws_reset(unsigned* ws, void* stream);
/* x = clamp(x0,-s,s)/s*sqrt_alpha_next + c*eps + sigma*noise   (noise may be NULL) */
int dawn_ddim_update(const float* x0, const float* eps, const float* s, const float* noise,
                     float sqrt_alpha_next, float c, float sigma, long n, float* x, void* stream);
/* ancestral (DDPM) step (p_sample MT:1113-1121): out = c1*clamp(x0,-s,s)/s + c2*x_t + std*noise   (noise may be NULL; s = s[0] of
 * dawn_select_finalize).  Bit-identical to dawn_ddim_update(x0, x_t, s, noise, c1, c2, std) into a separate buffer.  out may alias
 * x_t (the step updates in place); out must not alias x0 or noise. */
int dawn_ancestral_update(const float* x0, const float* x_t, const float* s, const float* noise, float c1, float c2, float std,
                          long n, float* out, void* stream);
/* ---- step tails of the x0 clipping modes that need no quantile (MT:1094-1107 / MT:1183-1196), ONE element-wise launch each:
 *   x0  = recip*x - recipm1*eps
 *   v   = clamp(x0, -1, 1)   clamp = 1: static thresholding (use_dynamic_thres = False, the reference's constructor default)
 *       = x0                 clamp = 0: no clipping (ddim_sample(clip_denoised=False)); DDIM only
 *   out = v*sqrt_alpha_next + c*eps + sigma*noise        (dawn_ddim_step_fixed)
 *   out = v*c1 + c2*x_t + std*noise                      (dawn_ancestral_step_fixed; clamp = 0 is an error: p_sample always clips)
 * noise may be NULL (term dropped); x0_out may be NULL (x0 is then never written to memory).  The roundings are those of dawn_ddim_x0
 * followed by dawn_ddim_update / dawn_ancestral_update, so clamp = 1 is bit-identical to that pair with s = 1, and clamp = 0 to
 * dawn_ddim_x0 followed by the update without the clamp.  Aliasing: out == x (x_t) is allowed (the step updates in place); out must
 * not overlap eps, noise or x0_out, nor x partially; x0_out must not overlap x, eps or noise: an error return, nothing launched.
 * 128-bit accesses when every pointer is 16-byte aligned, scalar otherwise; any n >= 0. */
int dawn_ddim_step_fixed(const float* x, const float* eps, const float* noise, float recip, float recipm1, float sqrt_alpha_next,
                         float c, float sigma, int clamp, long n, float* x0_out, float* out, void* stream);
int dawn_ancestral_step_fixed(const float* x_t, const float* eps, const float* noise, float recip, float recipm1, float c1, float c2,
                              float std, int clamp, long n, float* x0_out, float* out, void* stream);
/* ---- DPM-Solver++(2M) (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models"): a
 * second-order multistep solver in the data prediction, one evaluation per step like DDIM.  NOT in the reference: its values are THIS
 * definition, checked in fp64.  Quality against the number of steps on a trained checkpoint has not been measured by anyone; nothing
 * here says that fewer steps are as good as 50 DDIM steps.
 *   Steps are the DDIM time pairs (t, t_next) of ddim_time_pairs(S, timesteps).  The state at time t lies at the noise level the DDIM
 *   loop already uses, read from the fp32 table and then carried in fp64:
 *       abar = alphas_cumprod_prev[t], abar_n = alphas_cumprod_prev[t_next]
 *       alpha = sqrt(abar), sigma = sqrt(1 - abar), and alpha_n, sigma_n likewise.
 *   x0 is formed as everywhere else, recip[t]*x - recipm1[t]*eps with the non-_prev tables (the guided eps when guided), and clipped by
 *   the clip mode (dynamic at q, static, or none) as in the DDIM loop.  The clipped value v is what the solver sees and what the history
 *   keeps.  Per step i:
 *       rho = (sigma_n*alpha)/(alpha_n*sigma)       (= e^(-h); formed as this ratio so that sigma_n = 0 gives 0, not inf)
 *       A   = sigma_n/sigma      B0 = alpha_n*(1 - rho)      h = -ln rho   (only when sigma_n > 0)
 *       first order  (i = 0, or i = S-1 [lower-order final step], or sigma_n = 0, or order = 1):  b = B0,              c = 0
 *       second order (otherwise), r = h_prev / h:                                                b = B0*(1 + 1/(2r)), c = -B0/(2r)
 *       x_next = A*x + b*v + c*v_prev
 *   (a step whose h or h_prev is not positive -- two equal times, which ddim_time_pairs gives only for S close to timesteps -- is first
 *   order too: r would be 0 or infinite.)  A, b, c are rounded to fp32 once, on the host.  The last step has sigma_n = 0 (A = 0, b = 1):
 *   it returns v itself, the clipped x0, like the other loops.  No noise is drawn; ddim_sampling_eta is not read.
 * The two step tails.  Rounding order, the same in both and in their 128-bit and scalar paths (so every host is bit-identical):
 *       out = fma(c, v_prev, (A*x) + (b*v))         three roundings for (A*x) + (b*v), one more for the history term
 *   dawn_dpmpp_update      dynamic mode: v = clamp(x0,-s,s)/s with s = s[0] of dawn_select_finalize (one more rounding, the division)
 *   dawn_dpmpp_step_fixed  static (clamp = 1) and none (clamp = 0) in ONE launch: x0 = fma(recip, x, -(recipm1*eps)), the roundings of
 *                          dawn_ddim_x0 (as dawn_ddim_step_fixed); v = clamp(x0,-1,1) or x0; x0 does not go through memory
 *   so dawn_dpmpp_step_fixed equals dawn_ddim_x0 followed by dawn_dpmpp_update bit for bit at s = 1 (static) and with the clamp removed
 *   (none) -- the relation dawn_ddim_step_fixed has to dawn_ddim_x0 + dawn_ddim_update.  v_out = v (the next step's history) is always
 *   written.  v_prev = NULL drops the history term: hosts pass NULL whenever c == 0, because the history buffer is uninitialised on
 *   the first step and 0*NaN is NaN.  Aliasing: out == x and v_out == v_prev are allowed (each thread reads before it writes); any other
 *   overlap between an output and an input or the other output is an error return with a message, nothing launched.  128-bit accesses
 *   when every pointer is 16-byte aligned and n >= 4, scalar otherwise; any n >= 0. */
int dawn_dpmpp_update(const float* x0, const float* s, const float* x, const float* v_prev, float A, float b, float c, long n,
                      float* v_out, float* out, void* stream);
int dawn_dpmpp_step_fixed(const float* x, const float* eps, const float* v_prev, float recip, float recipm1, float A, float b, float c,
                          int clamp, long n, float* v_out, float* out, void* stream);
/* classifier-free guidance (Unet3D.forward_with_cond_scale MT:889-890): out = null + (cond-null)*scale */
int dawn_cfg_combine(const float* e_null, const float* e_cond, float scale, long n, float* out, void* stream);
/* cfg_combine then ddim_x0 in one pass: eps_out = null + (cond-null)*scale, x0_out = recip*x - recipm1*eps_out, and the 2048-bin
 * histogram of |x0| added into hist1 (zeroed by the caller) -- bit-identical to dawn_cfg_combine followed by dawn_ddim_x0.
 * eps_out may alias e_null or e_cond; x0_out must not alias x or eps_out. */
int dawn_cfg_x0(const float* e_null, const float* e_cond, float scale, const float* x, float recip, float recipm1, long n,
                float* eps_out, float* x0_out, unsigned* hist1, void* stream);
/* counter-based N(0,1): Philox4x32-10 keyed by seed, counter = (stream_id, global element index / 4) */
int dawn_philox_normal(float* out, int C, int F, int f0, int Ftotal, int hw, uint64_t seed, uint32_t stream_id,
                       void* stream);
/* ---- known-frame conditioning: the "replacement method" of video diffusion.  NOT in the reference: its values are THIS definition.
 * Quality on a trained checkpoint -- whether a continued clip drifts, whether a seam shows, which overlap is enough -- has not been
 * measured by anyone; nothing here claims it.
 *   Given a known latent `known` (3, F, h, w), a per-frame mask (frame f is known when mask[f] != 0) and a noise level (a_i, b_i) for
 *   i = 0 ... S, the latent that ENTERS step i of a sampler loop has its known frames set to the known latent at level i, and the latent
 *   the loop RETURNS has them at level S:
 *       x[:, f] = fadd(fmul(a_i, known[:, f]), fmul(b_i, z_i[:, f]))          for the known frames f
 *   each operation a separate fp32 rounding, no contraction.  Frames with mask[f] == 0 are neither read nor written by the replacement.
 *   Levels (host arithmetic, sampler.known_level_scalars): abar is read from the fp32 table, everything after it is fp64, a = sqrt(abar)
 *   and b = sqrt(1 - abar) are rounded to fp32 once.
 *       after a DDIM or DPM-Solver++ step      abar = alphas_cumprod_prev[t_next]   (the table and index the loop itself uses, MT:1170-1171)
 *       after an ancestral step                abar = alphas_cumprod_prev[t]
 *       level 0, DDIM and DPM-Solver++         abar = alphas_cumprod_prev[steps[0].t]
 *       level 0, ancestral                     abar = alphas_cumprod[timesteps - 1]
 *   The last step of every loop lands on alphas_cumprod_prev[0] = 1: a_S = 1, b_S = 0.  When b == 0 no noise is read or drawn and
 *   x = fmul(a, known), so the known frames of the result ARE the known latent, bit for bit -- chunks stitched over an overlap agree
 *   exactly there.
 *   Noise z_i: an injected tensor (the test hook, like `noises`) or the counter-based generator: exactly what
 *   dawn_philox_normal(seed, stream_id = 0x80000000 + i) writes at those elements (keyed by the GLOBAL element index: shard-invariant).
 *   These stream ids are disjoint from the step streams i + 1, the initial latent's stream 0 and PBnet's 0xFFFFFFFE / 0xFFFFFFFF.
 *   Unchanged by the replacement: x0, the dynamic-threshold quantile (over the whole clip, known frames included), the step tails, the
 *   DPM-Solver++ history (it holds x0 predictions) and the thresholds output.
 * dawn_known_replace: ONE launch on a (3, F, hw) latent, this rank's frames [f0, f0 + F) of a clip of Ftotal frames (f0 and Ftotal only
 * key the generator).  mask: F bytes of DEVICE memory.  The grid is laid out per frame: a block reads its frame's mask byte once and
 * leaves if it is zero.  noise != NULL: injected, (3, F, hw), any hw and any 4-byte alignment (128-bit accesses where the three
 * pointers allow, scalar elsewhere).  noise == NULL and b != 0: drawn inline for the known frames only; hw % 4 != 0 is then an error, as
 * in dawn_philox_normal.  b == 0: `noise` is not read, nothing is drawn.  Refused with a message, nothing launched: x, known or mask
 * NULL; x overlapping known or noise; F < 0, f0 < 0 or f0 + F > Ftotal.  F == 0 succeeds and launches nothing. */
int dawn_known_replace(float* x, const float* known, const unsigned char* mask, int F, int f0, int Ftotal, int hw, float a, float b,
                       const float* noise, uint64_t seed, uint32_t stream_id, void* stream);

/* ---- LFG flow decode, batched over the frames of a clip -----------------------------------------
 * (GEN = LFG/modules/generator.py:62-90, 138-171; blocks UTIL = LFG/modules/util.py:70-150; loop FD:372-385).
 * Activations are channels-last (rows = T*H*W, C) like everywhere else; every 3x3 convolution of the decoder goes
 * through dawn_conv_gemm.  Eval-mode BatchNorm is the per-channel affine a = gamma/sqrt(var+eps), b = beta - mean*a. */
/* out[row][c] = act(x[row][c]*a[c] + b[c]); act 0 none, 1 ReLU   (ResBlock2d norm+relu UTIL:83-88; x has row stride ld) */
int dawn_affine_act(const float* x, int ld, const float* a, const float* b, int act, float* out, long rows, int C,
                    void* stream);
/* DownBlock2d tail UTIL:129-133: out (F,H/2,W/2,C) = AvgPool2x2(ReLU(x*a+b)), x (F,H,W,C) */
int dawn_bn_relu_pool2(const float* x, const float* a, const float* b, float* out, int F, int H, int W, int C,
                       void* stream);
/* Generator.apply_optical GEN:71-90 on one level: skip (Hs,Ws,C) is the clip's single source feature map; grid =
 * two planes (x then y, `grid_plane` floats apart) of T frames (h,w) in grid_sample's normalised convention, conf (T,h,w)
 * the occlusion map; both are bilinearly resized to (Hs,Ws) (align_corners=False) when the sizes differ.
 *   out[t] = grid_sample(skip, flow[t]) * occ[t] + P * (1 - occ[t]),  P = prev[t]  or  relu(prev[t]*prev_a + prev_b)
 * (prev NULL: first term only).  up2 != 0 additionally applies the following UpBlock2d's nearest x2 upsampling
 * (UTIL:106): out is then (T,2Hs,2Ws,C). */
int dawn_warp_blend(const float* skip, int Hs, int Ws, int C, const float* grid, long grid_plane, const float* conf,
                    int T, int h, int w, const float* prev, const float* prev_a, const float* prev_b, int up2,
                    float* out, void* stream);
/* Generator.final (7x7, C->3) + sigmoid + the last apply_optical against the source image, and the `deformed` output
 * (GEN:152, 163-167).  x (T,H,W,C); w7 packed [49 taps][C/4][3 outputs][4 channels]; src (3,H,W) planar;
 * out_vid / warped_vid planar: channel ch of frame t at [ch*out_plane + t*H*W]  (== (3,T_total,H,W) slices). */
int dawn_final_conv_blend(const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                          const float* src, const float* grid, long grid_plane, const float* conf, int h, int w,
                          float* out_vid, float* warped_vid, long out_plane, void* stream);

/* ---- frame egress (UVG:383-397, `_process_output_frame` UVG:533-548) ---------------------------
 * vid = three fp32 planes (`plane` floats apart) of npix = T*H*W pixels each (a (3,T,H,W) clip) -> out (T,H,W,3) uint8:
 *   u8 = trunc(clip(float32(x + mean_c/255), 0, 1) * 255)   (numpy's arithmetic, bit-exact), channel order RGB, or
 * BGR (bgr != 0: cv2.cvtColor(RGB2BGR) for cv2.VideoWriter / imwrite).  mean0..2 = the caller's mean_c/255 as doubles. */
int dawn_frames_to_u8(const float* vid, long plane, long npix, double mean0, double mean1, double mean2, int bgr,
                      unsigned char* out, void* stream);
/* dawn_final_conv_blend with the egress above as its store: frames (T,H,W,3) uint8 receives, for every pixel and channel, exactly the
 * byte dawn_frames_to_u8 would make of the value dawn_final_conv_blend writes to out_vid (same kernel source up to the blended fp32
 * value, then the same u8 function); no fp32 frame is written, `deformed` is not produced.  Frame t of the launch goes to
 * frames + t*H*W*3.  W % 4 == 0 and a 4-byte aligned `frames` (rows leave as 4-byte stores): error otherwise, nothing launched. */
int dawn_final_conv_blend_u8(const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                             const float* src, const float* grid, long grid_plane, const float* conf, int h, int w,
                             double mean0, double mean1, double mean2, int bgr, unsigned char* frames, void* stream);

/* ---- yuv420p egress: the frames as planar YUV 4:2:0 (I420), what `-f rawvideo -pix_fmt yuv420p` and a Y4M FRAME read.
 * Input: the RGB bytes R,G,B of the egress above (u8 with mean_c/255, RGB order, i.e. dawn_frames_to_u8(..., bgr = 0)).
 * Output: BT.601 limited range in 8-bit fixed point, `>>` an arithmetic shift (floor):
 *   Y  = (( 66*R + 129*G +  25*B + 128) >> 8) + 16                       per pixel
 *   R' = (R00 + R01 + R10 + R11 + 2) >> 2   (same for G', B')            per 2x2 block, rows 2i,2i+1 x cols 2j,2j+1 (centre-sited)
 *   U  = ((-38*R' -  74*G' + 112*B' + 128) >> 8) + 128
 *   V  = ((112*R' -  94*G' -  18*B' + 128) >> 8) + 128
 * Y is in [16,235], U and V in [16,240] for every input (no clamp).  Layout: each frame contiguous, Y (H*W bytes), then U
 * ((H/2)*(W/2)), then V (the same); frames back to back: (T, 3*H*W/2) uint8.  H % 2 == 0, W % 4 == 0 and a non-NULL 4-byte aligned
 * output (Y rows leave as 4-byte stores, chroma as 2-byte stores): error otherwise, nothing launched.
 * dawn_frames_to_yuv420: vid = three fp32 planes (`plane` floats apart, a multiple of 4; 16-byte aligned) of a (3,T,H,W) clip. */
int dawn_frames_to_yuv420(const float* vid, long plane, int T, int H, int W, double mean0, double mean1, double mean2,
                          unsigned char* out, void* stream);
/* ---- yuv420p ingest (csrc/yuv_ingest.hip): the inverse of the egress above, for driving frames that arrive from a video decoder or a
 * .y4m file.  in = T I420 frames in the layout the egress writes (Y H*W bytes, then U and V (H/2)*(W/2) bytes each), frame t at
 * in + t*frame_stride bytes -> out (T,H,W,3) uint8 RGB frames, contiguous, as dawn_antialias_down reads them with in_kind = 1.
 * BT.601 limited range in 8-bit fixed point, `>>` an arithmetic shift (floor), chroma replicated over its 2x2 block (the centre siting
 * the egress assumes), clamp8(v) = min(max(v, 0), 255):
 *   C = Y - 16, D = U - 128, E = V - 128                       (D, E of the block's one chroma sample)
 *   R = clamp8((298*C         + 409*E + 128) >> 8)
 *   G = clamp8((298*C - 100*D - 208*E + 128) >> 8)
 *   B = clamp8((298*C + 516*D         + 128) >> 8)
 * Every byte value of Y, U, V is accepted (the clamp handles what lies outside the nominal ranges).  It is not the exact inverse of the
 * egress: that one averages chroma and rounds, so a round trip moves a byte by a few levels.
 * A work item converts a 2 x 8 pixel block (8-byte Y loads, 4-byte chroma loads, each output row as three 8-byte stores) when W % 8 == 0
 * and `in`, frame_stride and `out` are multiples of 8; otherwise a 2 x 4 block with loads that assume no alignment and each output row
 * as three 4-byte stores.  The bytes are the same on both paths.
 * Refused, with a message that names the argument and nothing launched: a NULL pointer, T < 1, H < 2 or odd, W < 4 or W % 4 != 0,
 * frame_stride < 3*H*W/2, an `out` that is not 4-byte aligned. */
int dawn_yuv420_to_frames(const unsigned char* in, long frame_stride, int T, int H, int W, unsigned char* out, void* stream);
/* dawn_final_conv_blend with the yuv420p egress defined above as its store: the same kernel source as dawn_final_conv_blend_u8 up to the
 * RGB bytes (bgr = 0), which stay in LDS and are converted there; no fp32 frame and no RGB byte is written.  Frame t of the launch goes
 * to frames + t*3*H*W/2. */
int dawn_final_conv_blend_yuv420(const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                                 const float* src, const float* grid, long grid_plane, const float* conf, int h, int w,
                                 double mean0, double mean1, double mean2, unsigned char* frames, void* stream);

/* ---- HuBERT audio features + 25 fps interpolation (UVG:202-250, 433-501; transformers.HubertModel with
 * feat_extract_norm = "layer", do_stable_layer_norm = True = hubert-large-ls960-ft).  Activations are (time, channels)
 * rows; the conv layers 1..6 and every Linear run through dawn_conv_gemm, the grouped positional conv through dawn_conv_gemm (one launch
 * per group on a zero-padded copy: the Python default) or dawn_hubert_pos_conv (one launch: the C-side stage further down). */
/* Wav2Vec2FeatureExtractor(do_normalize): out = (x - mean) / sqrt(var + 1e-7) over the utterance; stats2 = 2 doubles scratch */
int dawn_wave_normalize(const float* x, long n, double* stats2, float* out, void* stream);
/* conv_layers[0]: Conv1d(1, C, k, stride) (+ bias) of the waveform -> ((n - k) / stride + 1, C); w (C, k) */
int dawn_hubert_conv0(const float* x, long n, const float* w, const float* bias, int C, int k, int stride, float* out,
                      void* stream);
/* LayerNorm over the C channels of each row, affine; act 0 none, 2 exact (erf) GELU */
int dawn_ln_affine_act(const float* x, long rows, int C, const float* gamma, const float* beta, float eps, int act,
                       float* out, void* stream);
/* out = a + act(b) elementwise (a may be NULL); act 0 none, 2 exact GELU */
int dawn_add_act(const float* a, const float* b, int act, long n, float* out, void* stream);
/* HubertAttention core: qkv (T, 3*heads*64) = [q | k | v] (q unscaled), full softmax over the T frames, out (T, heads*64) */
int dawn_attn64(const float* qkv, int T, int heads, float* out, void* stream);
/* scipy interp1d(arange(n), y (n, C) fp32, kind="linear", axis=0)(xi) -> out (m, C) fp32; xi (m) doubles on the device */
int dawn_interp_linear(const float* y, long n, int C, const double* xi, long m, float* out, void* stream);
/* HubertPositionalConvEmbedding + the residual add that follows it, in one launch (grouped Conv1d(E, E, k, padding = k / 2, groups),
 * SamePad drop for even k, exact GELU, hidden + that):
 *   out[t][g gw + n] = hid[t][g gw + n] + gelu(bias[g gw + n] + sum_{j < k} sum_{c < gw} w[g][j][c][n] hid[t + j - k/2][g gw + c])
 * for t in [0, T); rows outside [0, T) read as zero; gw = E / groups, gw % 16 == 0, (63 + k) * (gw + 2) floats within 64 KB of LDS.
 * w = the per-group pack_kn images one after the other, contiguous as [groups][k gw / 4][gw][4]: element [g][q][n][e] is the weight of
 * input channel c = (4q + e) % gw at tap j = (4q + e) / gw (k index = tap * gw + c) for output channel n of group g.  hid, out (T, E)
 * dense, 16-byte aligned.  Exact fp32 on the matrix pipe; the sum order is fixed (no atomics): bit-identical run to run.  out may not
 * overlap hid (neighbouring rows are read): error, nothing launched. */
int dawn_hubert_pos_conv(const float* hid, int T, int E, int groups, int k, const float* w, const float* bias, float* out,
                         void* stream);

/* ---- PBnet pose / blink decoder (PBnet/src/models/architectures/transformerdecoder5.py:40-98, 120-166).
 * Attention core for heads of 32: out[i][h] = softmax_j(scale * rot(q_i,h) . rot(k_j,h) + bias[h][i][j]) v_j,h -- q / k / v rows with
 * strides ldq / ldk / ldv (column slices of a qkv tensor are fine), head h at columns [32h, 32h + 32); rotary embedding on the first
 * 2*nrot features of every head (interleaved pairs, position = row index) from cos / sin tables (max(Tq, Tk), nrot); bias
 * (heads, Tq, Tk) additive or NULL.  The rest of the decoder is dawn_linear / dawn_ln_affine_act / dawn_add_act. */
int dawn_attn_bias32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int Tq, int Tk, int heads,
                     const float* bias, const float* rot_cos, const float* rot_sin, int nrot, float scale, float* out, int ld_out,
                     void* stream);
/* The same attention with the eval-mode window as the key range instead of a -1e8 in the table: dawn_attn_bias32 with
 * bias[h][i][j] = bias_rel[h][j - i + win] for |j - i| <= win, and the keys with |j - i| > win absent for query i (in the dense form their
 * exp(-1e8 - max) is exactly 0 in fp32, so both compute the same function).  bias_rel (heads, 2*win + 1) or NULL.  O(Tq * win) time, no
 * table that grows with T; per-query key order ascending.  win < 0, Tq > Tk + win (a query row without a key), or the stride / nrot
 * conditions of dawn_attn_bias32: error return with a message, nothing launched. */
int dawn_attn_win32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int Tq, int Tk, int heads, int win,
                    const float* bias_rel, const float* rot_cos, const float* rot_sin, int nrot, float scale, float* out, int ld_out,
                    void* stream);

/* ---- whole-path entry points (C-side evaluator, csrc/dawn_ctx.hip) ----------------------------------
 * A host in any language runs the denoiser with these five calls (create, prepare, forward or sampler_run, destroy, plus the two
 * size queries) and turns its latent into frames with the decoder entries further down (dawn_decoder_create, dawn_decoder_encode,
 * dawn_decode_clip: sampler -> decode -> bytes without Python); the Python package keeps its own orchestration
 * (unet_forward.py, needed for the T-sharded path) and the GPU tests require both to agree bit for bit.
 *   dawn_ctx_create    packed weights (device pointers by name, layouts of pack.py) + architecture -> opaque ctx
 *   dawn_clip_prepare  per-clip tables (hoisted out of the DDIM loop: fea part of init_conv, condition -> k/v tables,
 *                      sigma-affine cross-attention tables, rotary + relative-position tables)   [FD:332-350, MT:1151,1167]
 *   dawn_unet_forward  one Unet3D.forward (null_cond_prob = 0) of one clip                       [MT:892-956]
 *   dawn_sampler_run   the DDIM loop: S x (forward, x0, dynamic-threshold quantile at 0.9, update)  [MT:1156-1208]
 *                      (other clipping modes / percentiles: dawn_sampler_run_clip, dawn_sampler_run_ancestral_clip below;
 *                      DPM-Solver++(2M) on the same time pairs, not in the reference: dawn_sampler_run_dpmpp)
 * No allocation, no synchronisation: the caller owns the clip memory (dawn_clip_bytes) and the workspace
 * (dawn_workspace_bytes); launches go to `stream` and to one ctx-owned side stream forked / joined with events.
 * One host thread per ctx.  Single GPU (the T-shard exchanges live in the Python host, tshard.py). */
typedef struct dawn_ctx dawn_ctx;
typedef struct dawn_unet_cfg {
    int dim;                 /* base width (64) */
    int n_levels;            /* len(dim_mults) */
    int dim_mults[8];        /* (1, 2, 4, 8) */
    int fea_ch;              /* frame-invariant input channels (256 fea + 16 bbox = 272) */
    int cond_aud, cond_pose, cond_eye;   /* condition columns [aud | pose | eye] (MT:426-428) */
    int win;                 /* local-attention half window (40) */
} dawn_unet_cfg;
typedef struct dawn_named_ptr { const char* name; const void* ptr; } dawn_named_ptr;
/* weight names = the fields of pack.PackedUNet, dotted: "w3" "wfea" "b_init" "rel_emb" "rot_freqs" "sin_freqs" "t_w1" "t_b1"
 * "t_w2" "t_b2" "film_w" "film_b" "wg" "bg" "wo" "bo"; attention layers "<init_tattn|downs.L.sla|downs.L.tattn|mid.sattn|
 * mid.tattn|ups.L.sla|ups.L.tattn>.<wqkv|wout|bout|wqkv_s|wout_s|wout_sp>"; ResBlocks "<downs.L.rb1|...|mid.rb1|mid.rb2|
 * head_g|head_o>.<w1|b1|g1|be1|w2|b2|g2|be2|wr|br|w1s|w2s|wrs|wq|wqs|q_scale|g3|wo.B|wos.B|mlp_w.B|mlp_b.B|kv_w.B|k_scale.B|
 * null_kv.B>" (B = 0..2: pose, aud, eye); "downs.L.down.<w|b|ws>", "ups.L.up.<w|b|ws>" (ws optional: pack_bf3 image(s) of the
 * resampling convolution for the split pipeline; dawn_pytorch_amd/ctx.py builds the table).
 * "ups.L.up.w" is four phase blocks (py, px) of 2x2 taps (ty, tx), each [4 C / 4][C][4] with k = (2 ty + tx) C + c; tap 0 sits on the
 * input pixel, tap 1 one pixel before it (phase bit 0) or after it (phase bit 1).  use_deconv=True checkpoints (ups.L.4.weight,
 * (C, C, 1, 4, 4)): tap t of phase bit p is kernel row / column ((1, 3), (2, 0))[p][t] (pack.deconv_w_kn_phases).  use_deconv=False
 * checkpoints (ups.L.4.1.weight, (C, C, 1, 3, 3): nearest x2 upsample + 3x3 conv, MT:169-172): the host FOLDS the 3x3 kernel, per
 * axis tap 0 = w[1] + w[2], tap 1 = w[0] for phase bit 0 and tap 0 = w[0] + w[1], tap 1 = w[2] for phase bit 1, a 2-D tap being
 * the sum of the kernel entries of the product set (pack.upconv_w_kn_phases: summed in fp64, rounded once), and sets
 * DAWN_OPT_UP_BORDER from the checkpoint's padding_mode. */
int dawn_ctx_create(const dawn_unet_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_ctx** out);
void dawn_ctx_destroy(dawn_ctx* ctx);
enum { DAWN_OPT_CONV_POLICY = 1, DAWN_OPT_TEMPORAL_FLAGS = 2, DAWN_OPT_OVERLAP = 3, DAWN_OPT_PROFILE = 4, DAWN_OPT_LONG_CLIP_FRAMES = 5,
       DAWN_OPT_UP_BORDER = 6, DAWN_OPT_FOLD_HEADS = 7 };
/* tuning state lives in the ctx: conv policy bits (dawn_conv_desc.policy), temporal-layer kernel family, two-stream
 * overlap on/off, per-launch HIP events around every dawn_conv_gemm (read with dawn_ctx_profile_read), the clip length above which an
 * evaluation runs in its memory-lean form (default 4096 frames: qkv tensors of the unfused attention levels per frame segment, the
 * heads' skip recomputed, the heads one after the other: 4.65 instead of 7.8 MB of workspace per frame at 256x256 for ~3 % of time;
 * set it BEFORE dawn_workspace_bytes); DAWN_OPT_UP_BORDER = dawn_conv_desc.border of the Upsample launches (0 zero: the default,
 * and the only value for use_deconv=True weights; 1 edge: padding_mode reflect / replicate; 2 wrap: circular; anything else is an
 * error) -- it reaches dawn_unet_forward, the guided and sharded forwards and every dawn_sampler_run* entry; DAWN_OPT_FOLD_HEADS
 * (default 1; set it BEFORE dawn_workspace_bytes): the heads' res_conv folded into the output projection, the end of an evaluation is
 * one dawn_heads_eps launch (0: res_conv through dawn_conv_gemm, then dawn_head_out).  The folded (3, 2 dim) matrix is computed in
 * dawn_ctx_create with dawn_fold_heads and lives in a small device buffer that the ctx owns (the one exception to "no allocation") */
int dawn_ctx_set_option(dawn_ctx* ctx, int option, int value);
size_t dawn_clip_bytes(dawn_ctx* ctx, int F, int h, int w);
size_t dawn_workspace_bytes(dawn_ctx* ctx, int F, int h, int w);      /* covers prepare, forward and sampler_run */
/* fea272 (fea_ch, h, w) reference layout; cond (F, cond_dim) with row stride ld_cond; rot_cos / rot_sin optional
 * (F + 2 win, 16) tables (NULL: computed on the device from the checkpoint's `freqs`) */
int dawn_clip_prepare(dawn_ctx* ctx, int F, int h, int w, const float* fea272, const float* cond, int ld_cond,
                      const float* rot_cos, const float* rot_sin, void* clip_mem, size_t clip_bytes, void* workspace,
                      size_t workspace_bytes, void* stream);
/* x3, eps_out: (3, F, h, w) latent / predicted noise in the reference layout; t = the integer diffusion time */
int dawn_unet_forward(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const float* x3, float t,
                      float* eps_out, void* workspace, size_t workspace_bytes, void* stream);
typedef struct dawn_ddim_step {          /* per-step scalars of MT:1170-1205 (host arithmetic of the schedule tables) */
    int t, t_next;
    float recip, recipm1;                /* sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t] */
    float sqrt_alpha_next, c, sigma;
} dawn_ddim_step;
/* x_init -> x_out (3, F, h, w).  Noise of step i (only when t_next > 0): noises[i] when `noises` is given, else the
 * counter-based generator (seed, stream i + 1).  thresholds (optional, 2 S floats): [max(1, q), q] of every step. */
int dawn_sampler_run(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const float* x_init, int S,
                     const dawn_ddim_step* steps, uint64_t seed, const float* const* noises, float* x_out,
                     float* thresholds, void* workspace, size_t workspace_bytes, void* stream);
/* ---- T-shard through the C ABI.  One rank of a clip sharded along T over `world` processes / GPUs: this rank
 * owns the global frames [rank*F, (rank+1)*F) of a clip of world*F frames; clip_mem is prepared (dawn_clip_prepare) with THIS rank's
 * F rows of the condition.  The path has exactly three exchanges; the host supplies them as callbacks (RCCL / MPI / anything):
 *   halo_begin   a temporal layer's input as frame-major rows [hl lower-halo frames | F own frames | hh upper-halo frames] of
 *                frame_floats floats each, own frames in place: send the own edge frames the neighbours need, receive the halo
 *                frames (global frames [rank*F - hl, rank*F) and [(rank+1)*F, (rank+1)*F + hh); hl, hh <= win, 0 at the clip ends;
 *                a halo wider than a shard spans several ranks).  May return before the transfer completes;
 *   halo_end     make `stream` wait for the transfer posted by the last halo_begin (the evaluator launches the work that only
 *                reads own frames between the two);
 *   allreduce_*  in-place sum / min over the ranks: 16 fp64 GroupNorm sums (40 per evaluation), the radix-select histograms
 *                (2048 / 1024 / 1024 u32) and one u32 minimum per DDIM step.
 * Every callback is stream-ordered: it sees the work already enqueued on `stream`, and work enqueued on `stream` after it sees
 * its result.  Return 0 or a negative error code (the evaluation stops and returns it).  NULL comm = dawn_unet_forward. */
typedef struct dawn_shard_comm {
    void* user;
    int rank, world;
    int (*halo_begin)(void* user, float* xe, int hl, int F, int hh, long frame_floats, void* stream);
    int (*halo_end)(void* user, void* stream);
    int (*allreduce_sum_f64)(void* user, double* buf, int n, void* stream);
    int (*allreduce_sum_u32)(void* user, unsigned* buf, int n, void* stream);
    int (*allreduce_min_u32)(void* user, unsigned* buf, int n, void* stream);
} dawn_shard_comm;
size_t dawn_workspace_bytes_sharded(dawn_ctx* ctx, int F, int h, int w, int rank, int world);
int dawn_unet_forward_sharded(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const float* x3, float t, float* eps_out,
                              void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm, void* stream);
/* noise of step i: noises[i] (this rank's frames) or the counter-based generator keyed by the GLOBAL element index (shard-invariant);
 * the 0.9-quantile is over the whole clip (histogram all-reduces) */
int dawn_sampler_run_sharded(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const float* x_init, int S,
                             const dawn_ddim_step* steps, uint64_t seed, const float* const* noises, float* x_out,
                             float* thresholds, void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm, void* stream);
/* ---- classifier-free guidance on the whole path (Unet3D.forward_with_cond_scale MT:879-890, cond_scale != 1).  null_clip_mem is a clip
 * prepared by dawn_clip_prepare from the SAME fea272 with an all-zero condition (learn_null_cond = False, MT:920): ld_cond = 0 with a
 * single zero row of cond_dim floats is enough.  One guided evaluation runs the condition-free prefix ONCE (init conv, init temporal
 * layer with its halo exchange, conv1 + GroupNorm statistics of downs[0].rb1), then the conditional and the null branch, then
 * eps = null + (cond - null) * cond_scale; every result is bit-identical to two dawn_unet_forward calls + dawn_cfg_combine.
 * comm = NULL: single GPU (rank 0, world 1 for the workspace query). */
size_t dawn_workspace_bytes_guided(dawn_ctx* ctx, int F, int h, int w, int rank, int world);
int dawn_unet_forward_guided(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem, const float* x3, float t,
                             float cond_scale, float* eps_out, void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm,
                             void* stream);
/* dawn_sampler_run(_sharded) with every evaluation guided; guided eps, x0 and the first quantile histogram come from one dawn_cfg_x0 launch */
int dawn_sampler_run_guided(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem, float cond_scale,
                            const float* x_init, int S, const dawn_ddim_step* steps, uint64_t seed, const float* const* noises,
                            float* x_out, float* thresholds, void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm,
                            void* stream);
/* ---- ancestral sampling (GaussianDiffusion.p_sample_loop MT:1124-1135, taken when sampling_timesteps >= timesteps): one evaluation per
 * integer time t = timesteps-1 ... 0, each followed by the same dynamic-threshold quantile as DDIM and the posterior step
 * x = c1 * clamp(x0,-s,s)/s + c2 * x + std * noise (dawn_ancestral_update, in place).  Scalars are host arithmetic of the fp32 schedule
 * tables: c1 / c2 = posterior_mean_coef1 / 2 [t], std = exp(0.5 * posterior_log_variance_clipped[t]) in fp32. */
typedef struct dawn_ancestral_step {
    int t;
    float recip, recipm1;                /* sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t] */
    float c1, c2, std;
} dawn_ancestral_step;
/* ONE entry for every form: guided (as dawn_sampler_run_guided) when null_clip_mem != NULL and cond_scale != 1, T-sharded (as
 * dawn_sampler_run_sharded) when comm != NULL.  Noise of step i only when steps[i].t > 0: noises[i] when `noises` is given (S - 1
 * entries suffice), else the counter-based generator (seed, stream i + 1).  thresholds (optional, 2 S floats): [max(1, q), q] of every
 * step.  Workspace: the existing queries cover this entry -- dawn_workspace_bytes (single GPU), dawn_workspace_bytes_sharded (comm),
 * dawn_workspace_bytes_guided (guided, either form); the loop keeps the same sampler state as the DDIM entries. */
int dawn_sampler_run_ancestral(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem, float cond_scale,
                               const float* x_init, int S, const dawn_ancestral_step* steps, uint64_t seed, const float* const* noises,
                               float* x_out, float* thresholds, void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm,
                               void* stream);
/* ---- x0 clipping modes of the whole-loop entries (MT:1094-1107 in p_mean_variance, MT:1183-1196 in ddim_sample).
 *   DAWN_CLIP_DYNAMIC  s = max(1, quantile_q(|x0|)) over the whole clip, x0 = clamp(x0,-s,s)/s     (use_dynamic_thres = True)
 *   DAWN_CLIP_STATIC   x0 = clamp(x0,-1,1)                            (use_dynamic_thres = False, the reference's constructor default)
 *   DAWN_CLIP_NONE     x0 unchanged                                   (ddim_sample(clip_denoised=False); DDIM steps only)
 * q is read for DAWN_CLIP_DYNAMIC only and must lie in [0, 1]; the rank is q * (n - 1) in fp32 up to 2^24 elements (torch.quantile forms
 * it in the input dtype), in fp64 above.  STATIC / NONE run the evaluation (a guided one ends in dawn_cfg_combine) and then ONE
 * dawn_ddim_step_fixed / dawn_ancestral_step_fixed launch per step: no histogram, no selection pass and, T-sharded, none of the four
 * allreduce_sum_u32 / allreduce_min_u32 calls of the dynamic step tail (those two callbacks may then be NULL). */
enum { DAWN_CLIP_DYNAMIC = 0, DAWN_CLIP_STATIC = 1, DAWN_CLIP_NONE = 2 };
typedef struct dawn_clip_mode { int kind; double q; } dawn_clip_mode;
/* dawn_sampler_run / _sharded / _guided in one entry (guided when null_clip_mem != NULL and cond_scale != 1, T-sharded when comm !=
 * NULL) with the clipping mode; clip = NULL means {DAWN_CLIP_DYNAMIC, 0.9}, with which the result is bit-identical to those entries.
 * thresholds (optional, 2 S floats): DYNAMIC [max(1, q-quantile), q-quantile] of every step; STATIC [1, 1] of every step; NONE leaves
 * the rows untouched.  An unknown kind, a q outside [0, 1] or NaN: error return with a message, nothing launched.  Workspace: the
 * existing queries, as for dawn_sampler_run_ancestral. */
int dawn_sampler_run_clip(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem, float cond_scale,
                          const float* x_init, int S, const dawn_ddim_step* steps, uint64_t seed, const float* const* noises,
                          float* x_out, float* thresholds, void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm,
                          const dawn_clip_mode* clip, void* stream);
/* dawn_sampler_run_ancestral with the clipping mode (DAWN_CLIP_NONE is an error here: the reference's p_sample always clips) */
int dawn_sampler_run_ancestral_clip(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem,
                                    float cond_scale, const float* x_init, int S, const dawn_ancestral_step* steps, uint64_t seed,
                                    const float* const* noises, float* x_out, float* thresholds, void* workspace,
                                    size_t workspace_bytes, const dawn_shard_comm* comm, const dawn_clip_mode* clip, void* stream);
/* ---- DPM-Solver++(2M) on the whole path (the definition stands with dawn_dpmpp_update above; host arithmetic of the steps:
 * sampler.dpmpp_step_scalars).  a, b, c: the fp32-rounded A, b, c of the definition; c == 0 marks a first-order step. */
typedef struct dawn_dpmpp_step { int t; float recip, recipm1; float a, b, c; } dawn_dpmpp_step;
/* ONE entry for every form: guided when null_clip_mem != NULL and cond_scale != 1, T-sharded when comm != NULL, clip = NULL means
 * {DAWN_CLIP_DYNAMIC, 0.9}.  Per step: the evaluation, x0, the threshold selection (dynamic only), then dawn_dpmpp_update (dynamic) or
 * dawn_dpmpp_step_fixed (static / none) with v_prev = NULL when steps[i].c == 0.  Deterministic: no seed, no noises.  The `noise` latent
 * of the sampler state carries the one-step history v_prev, so the existing workspace queries cover this entry (dawn_workspace_bytes,
 * dawn_workspace_bytes_sharded, dawn_workspace_bytes_guided).  T-sharded, the dynamic mode keeps the four histogram / minimum
 * all-reduces per step; static and none need none (allreduce_sum_u32 / allreduce_min_u32 may then be NULL).  thresholds as for
 * dawn_sampler_run_clip.  steps[0].c != 0 (no history exists yet) is refused before the first launch. */
int dawn_sampler_run_dpmpp(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem, float cond_scale,
                           const float* x_init, int S, const dawn_dpmpp_step* steps, float* x_out, float* thresholds, void* workspace,
                           size_t workspace_bytes, const dawn_shard_comm* comm, const dawn_clip_mode* clip, void* stream);
/* ---- known-frame conditioning on the whole path (the definition stands with dawn_known_replace above).  ONE entry for every loop:
 * `solver` names the kind of `steps` (DAWN_SOLVER_DDIM: dawn_ddim_step[S], DAWN_SOLVER_ANCESTRAL: dawn_ancestral_step[S],
 * DAWN_SOLVER_DPMPP: dawn_dpmpp_step[S]; for DPMPP `noises` is not read and `seed` keys the known-frame noise only).  Guided when null_clip_mem != NULL and cond_scale != 1,
 * T-sharded when comm != NULL, clip = NULL means {DAWN_CLIP_DYNAMIC, 0.9}; every other argument as in the entry of that solver.
 *   known        (3, F, h, w) device, this rank's frames of the known latent (frames outside the mask are never read)
 *   known_mask   F bytes, device
 *   known_ab     host, 2 (S + 1) floats: a_0, b_0, ..., a_S, b_S (sampler.known_level_scalars)
 *   known_noises optional, host array of S + 1 device pointers: z_i (3, F, h, w) of every level with b_i != 0 (the others may be NULL);
 *                NULL: the counter-based generator (seed, stream 0x80000000 + i), keyed by the global element index
 * The replacement runs on the copy of x_init (level 0) and after every step tail (level i + 1), one dawn_known_replace launch each.
 * known == NULL: the result is bit-identical to the existing entry of that solver (known_mask / known_ab / known_noises are not read).
 * known != NULL with known_mask or known_ab NULL, or an unknown solver: error return with a message, nothing launched.  The known latent
 * is the caller's buffer, so the existing workspace queries cover this entry too. */
enum { DAWN_SOLVER_DDIM = 0, DAWN_SOLVER_ANCESTRAL = 1, DAWN_SOLVER_DPMPP = 2 };
int dawn_sampler_run_known(dawn_ctx* ctx, int F, int h, int w, const void* clip_mem, const void* null_clip_mem, float cond_scale,
                           const float* x_init, int S, int solver, const void* steps, uint64_t seed, const float* const* noises,
                           float* x_out, float* thresholds, void* workspace, size_t workspace_bytes, const dawn_shard_comm* comm,
                           const dawn_clip_mode* clip, const float* known, const unsigned char* known_mask, const float* known_ab,
                           const float* const* known_noises, void* stream);
/* ---- chunked generation of a long clip: the plan (pure host arithmetic, no GPU; sampler.chunk_plan is the same function).  A clip of T
 * frames is sampled as chunks of F frames of which the first K (the overlap, 1 <= K < F) are already generated and pinned as the known
 * set.  T <= F: one chunk (0, T frames, known 0).  T > F: chunks of exactly F frames start at 0, F - K, 2 (F - K), ... while
 * start + F < T; the last chunk starts at T - F and its known count is however many of its frames are already generated (between K
 * and F - 1).  Every chunk has ONE shape: one workspace, one clip_mem size, one captured graph.  Chunk j emits the frames
 * [starts[j] + known[j], starts[j] + F).  Returns the number of chunks and writes the first min(n, max_chunks) entries of starts /
 * known (either may be NULL); a precondition that fails (T < 1, F < 1, K < 1 or K >= F) returns a negative code with a message.  A C host
 * loops over the plan with dawn_clip_prepare + dawn_sampler_run_known itself (INTEGRATION.md has the loop). */
int dawn_chunk_plan(int T, int F, int K, int* starts, int* known, int max_chunks);
/* ---- SURVEY 8(f) N1 + N2 as a whole path: the LFG flow decode of a sampled clip, down to uint8 frames (csrc/dawn_decoder.hip).
 * The same launch sequence as dawn-pytorch_amd/flow_decoder.py (FlowDecoder.encode / _decode_frames / decode_clip), results bit-identical
 * to it (tests/test_hip_decode_u8.py).  Same contract as dawn_ctx: opaque handle, device pointers by name, caller-owned memory, every
 * launch on `stream`, no allocation, no synchronisation.  The decoder is immutable after creation (the size queries are pure functions).
 *   dawn_decoder_create   packed weights + topology -> opaque decoder
 *   dawn_decoder_encode   once per clip: source image -> encoder skips (GEN:140-146) and, optionally, `fea` for dawn_clip_prepare
 *   dawn_decode_clip      the sampler's latent (3,T,h,w) -> fp32 clips and / or (T,H,W,3) uint8 frames, chunk by chunk
 * Weight names = the packed fields FlowDecoder.__init__ builds (i = block index; <conv> = w | ws | bias, `ws` = the pack_bf3 image,
 * optional, absent when 9 * Cin % 16 != 0):
 *   "first_w3" (147, C0)   "first_bias" (C0)   "first.a" "first.b" (C0)                      first 7x7 conv, its BatchNorm as a / b
 *   "downs.i.<conv>" "downs.i.a" "downs.i.b"                                                  DownBlock2d i: 3x3 conv, BatchNorm
 *   "bott.i.a1" "bott.i.b1" "bott.i.c1.<conv>" "bott.i.a2" "bott.i.b2" "bott.i.c2.<conv>"     ResBlock2d i
 *   "ups.i.<conv>" "ups.i.a" "ups.i.b"                                                        UpBlock2d i
 *   "final_w7" [49][C0/4][3][4]   "final_bias" (3)                                           final 7x7 conv */
typedef struct dawn_decoder dawn_decoder;
typedef struct dawn_decoder_cfg {
    int n_down;              /* DownBlock2d count = UpBlock2d count (2) */
    int n_bottleneck;        /* ResBlock2d count (6) */
    int widths[8];           /* widths[0] = channels after the first conv (64), widths[i] = after down block i - 1 (128, 256);
                                up block i maps widths[n_down - i] -> widths[n_down - i - 1].  Multiples of 8 */
} dawn_decoder_cfg;
/* a missing name or an unusable width: error return with a message, *out untouched */
int dawn_decoder_create(const dawn_decoder_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_decoder** out);
void dawn_decoder_destroy(dawn_decoder* dec);
/* bytes of the per-clip skip memory (encoder outputs at every level) for H x W images (multiples of 2^n_down; 0 otherwise) */
size_t dawn_decoder_skip_bytes(dawn_decoder* dec, int H, int W);
/* bytes of the workspace that covers dawn_decoder_encode and dawn_decode_clip with chunks of up to `chunk` frames */
size_t dawn_decoder_workspace_bytes(dawn_decoder* dec, int H, int W, int chunk);
/* img3 (3,H,W) fp32 planar in [0,1] -> skip_mem; fea_out optional: (widths[n_down], H/2^n, W/2^n) reference layout = Generator.compute_fea
 * (GEN:132-136), the first 256 channels of dawn_clip_prepare's fea272 */
int dawn_decoder_encode(dawn_decoder* dec, int H, int W, const float* img3, void* skip_mem, size_t skip_bytes, float* fea_out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* latent: the (3,T,h,w) output of any dawn_sampler_run*, taken as is -- three planes `latent_plane` floats apart: x and y of the
 * sampling grid, then p with occlusion = (p + 1) * 0.5 (two fp32 roundings, as torch evaluates FD:360), formed per chunk into the
 * workspace.  Frames are decoded `chunk` at a time (the launch sequence of FlowDecoder._decode_frames).  Outputs, each optional:
 *   out_vid, warped_vid   fp32 (3,T,H,W) planar, channel planes out_plane floats apart (both or neither);
 *   frames_u8             (T,H,W,3) uint8: the egress of dawn_frames_to_u8 with mean3 = 3 HOST doubles (mean_c / 255; NULL = 0) and
 *                         the bgr flag.  Alone: every chunk ends in dawn_final_conv_blend_u8 and no fp32 frame is written anywhere;
 *                         with the fp32 pair: dawn_final_conv_blend, then dawn_frames_to_u8 on the chunk.
 * Neither output, W % 4 != 0 with frames_u8, a short workspace: error return with a message, nothing launched. */
int dawn_decode_clip(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                     const float* latent, long latent_plane, int chunk, float* out_vid, float* warped_vid, long out_plane,
                     unsigned char* frames_u8, const double* mean3, int bgr, void* workspace, size_t workspace_bytes, void* stream);
/* the same for a host that holds the occlusion map already: grid = two planes (T,h,w) grid_plane floats apart, conf (T,h,w) */
int dawn_decode_clip_conf(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                          const float* grid, long grid_plane, const float* conf, int chunk, float* out_vid, float* warped_vid,
                          long out_plane, unsigned char* frames_u8, const double* mean3, int bgr, void* workspace,
                          size_t workspace_bytes, void* stream);
/* dawn_decode_clip / dawn_decode_clip_conf with yuv420p frames as the one output: the same launch sequence, every chunk ending in
 * dawn_final_conv_blend_yuv420; no fp32 frame and no RGB byte is written anywhere.  frames_yuv420 = (T, 3*H*W/2) uint8, I420, the
 * definition stated at dawn_frames_to_yuv420 (Y = ((66R + 129G + 25B + 128) >> 8) + 16; U, V from the rounded 2x2 box average of R, G, B:
 * U = ((-38R' - 74G' + 112B' + 128) >> 8) + 128, V = ((112R' - 94G' - 18B' + 128) >> 8) + 128; BT.601 limited range) on the RGB bytes
 * of frames_u8 with bgr = 0.  The workspace is the one dawn_decoder_workspace_bytes states (no more than the frames_u8-alone path).
 * Odd H, W % 4 != 0, a NULL or unaligned output, a short workspace: error return with a message, nothing launched. */
int dawn_decode_clip_yuv420(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                            const float* latent, long latent_plane, int chunk, unsigned char* frames_yuv420, const double* mean3,
                            void* workspace, size_t workspace_bytes, void* stream);
int dawn_decode_clip_conf_yuv420(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                                 const float* grid, long grid_plane, const float* conf, int chunk, unsigned char* frames_yuv420,
                                 const double* mean3, void* workspace, size_t workspace_bytes, void* stream);
/* ---- SURVEY 8(f) N3 as a whole path: the HuBERT audio-feature stage from raw 16 kHz samples to the 25 fps feature rows of `cond`
 * (csrc/dawn_hubert.hip).  The launch sequence of dawn-pytorch_amd/hubert.py (HubertFeatures.encode / get_hubert_from_16k_speech /
 * interpolate_25fps = VideoGenerator.process_audio, UVG:202-250, 433-501) through the per-op entries of this library, with the
 * positional block as the one dawn_hubert_pos_conv launch.  Same contract as dawn_decoder: opaque handle, device pointers by name,
 * caller-owned workspace, every launch on `stream`, no allocation, no synchronisation; an error return comes with a dawn_last_error
 * message and nothing launched.  The handle is immutable after creation (the size queries are pure functions).
 * Weight names = the fields HubertFeatures.__init__ builds (i = layer index; every matrix a pack_kn image):
 *   "conv.0.w" (conv_dim, conv_k[0])   "conv.i.w" [conv_k[i] conv_dim / 4][conv_dim][4] (i >= 1)   "conv.i.b" (optional: conv_bias)
 *   "conv.i.g" "conv.i.be"                                      feature-extractor conv i and the LayerNorm after it
 *   "fp.g" "fp.b" (conv_dim)   "fp.w" [conv_dim / 4][hidden][4]   "fp.bias"                       feature projection
 *   "pos.w" [pos_groups][pos_k gw / 4][gw][4]   "pos.b" (hidden)                                  positional conv (weight norm folded)
 *   "layers.i.ln1.g" "layers.i.ln1.b" "layers.i.wqkv" [hidden / 4][3 hidden][4] "layers.i.bqkv" "layers.i.wo" "layers.i.bo"
 *   "layers.i.ln2.g" "layers.i.ln2.b" "layers.i.w1" "layers.i.b1" (intermediate) "layers.i.w2" "layers.i.b2"   encoder layer i (pre-LN)
 *   "enc_ln.g" "enc_ln.b"                                                                         final LayerNorm */
typedef struct dawn_hubert dawn_hubert;
typedef struct dawn_hubert_cfg {
    int n_conv;                          /* feature-extractor conv layers (7), at most 8 */
    int conv_k[8], conv_stride[8];       /* (10,3,3,3,3,2,2) / (5,2,2,2,2,2,2) */
    int conv_dim;                        /* their width (512), a multiple of 4 */
    int hidden;                          /* E (1024) = 64 * heads */
    int heads;                           /* 16 */
    int intermediate;                    /* FFN width (4096) */
    int n_layers;                        /* encoder layers (24) */
    int pos_k, pos_groups;               /* positional conv: taps (128), groups (16); gw = hidden / pos_groups, gw % 16 == 0 */
    float eps;                           /* layer_norm_eps (1e-5) */
} dawn_hubert_cfg;
/* a missing name, hidden != 64 * heads, gw % 16 != 0 or any other unusable size: error return with a message, *out untouched */
int dawn_hubert_create(const dawn_hubert_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_hubert** out);
void dawn_hubert_destroy(dawn_hubert* hub);
/* rows the conv stack makes of n_samples samples (host code; 0 when they are fewer than the stack needs) */
long dawn_hubert_conv_frames(const dawn_hubert* hub, long n_samples);
/* the segment plan of UVG:466-501 + 229-236 (host code): segments of 320000 samples plus 80 of right context, clamped to n_samples, the
 * last one if it holds at least 400.  Returns the number of segments (> 0) and writes three numbers per segment -- first sample, samples,
 * rows it encodes to (segment s starts at the sum of the rows before it) -- plus expected_T = (n_samples - 80) / 320 and
 * num_frames = (long)((double)n_samples / 16000.0 * 25.0) (either pointer may be NULL).  Returns a negative error code with a message
 * for n_samples < 400, more than max_segments segments, or a row total that differs from expected_T by more than one. */
int dawn_hubert_segments(const dawn_hubert* hub, long n_samples, long* start_len_rows, int max_segments, long* expected_T,
                         long* num_frames);
/* bytes of the workspace that covers dawn_hubert_features of n_samples samples and dawn_hubert_encode of min(n_samples, 320080) */
size_t dawn_hubert_workspace_bytes(const dawn_hubert* hub, long n_samples);
/* HubertModel.forward on one segment: input_values = n normalised samples (n <= 320080: one segment of the plan above) ->
 * last_hidden_state, hidden_out (dawn_hubert_conv_frames(n), hidden) */
int dawn_hubert_encode(dawn_hubert* hub, const float* input_values, long n, float* hidden_out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* all of process_audio: speech = n raw fp32 samples on the device -> dawn_wave_normalize -> every segment of the plan encoded straight to
 * its row offset of the hidden block (no concatenation; a surplus row is not computed, a missing one is a zero row) ->
 * dawn_interp_linear at numpy's linspace(0, expected_T - 1, num_frames) (filled on the device: xi[i] = (double)i * step,
 * step = (double)(expected_T - 1) / (num_frames - 1), the last entry expected_T - 1 exactly; num_frames == 1: xi = {0}).
 * hidden_out optional (expected_T, hidden): NULL keeps the block in the workspace; features_out (num_frames, hidden) = the audio rows
 * of `cond`.  n < 400, num_frames == 0, expected_T < 2, a short workspace: error return with a message, nothing launched. */
int dawn_hubert_features(dawn_hubert* hub, const float* speech, long n, float* hidden_out, float* features_out, void* workspace,
                         size_t workspace_bytes, void* stream);
/* ---- SURVEY 8(f) N4 as a whole path: the PBnet pose / blink stage (csrc/dawn_pbnet.hip).  The launch sequence of
 * dawn-pytorch_amd/pbnet.py (PoseBlinkGenerator._decode_one = Decoder.forward for one sample with all frames valid; pose_blink_stage =
 * UVG:252-302) through the per-op entries of this library, with dawn_attn_win32 as the attention: no table grows faster than T.  Same
 * contract as dawn_hubert: opaque handle, device pointers by name, caller-owned workspace, every launch on `stream`, no allocation, no
 * synchronisation; an error return comes with a dawn_last_error message and nothing launched.  The handle is immutable after creation.
 * Weight names = the decoder's state_dict keys as PoseBlinkGenerator holds them (fp32, row-major (out, in), L = layer index):
 *   "firstposeEmbedding.weight|bias" (d, in_dim)   "audioEmbedding.weight|bias" (latent_dim, audio_dim)
 *   "ztimelinear.weight|bias" (d, d + 2 latent_dim)   "init_proj.bias" (d)   "finallayer.weight|bias" (in_dim, d)
 *   "init_temporal_attn.fn.norm.gamma|beta" (d)   "init_temporal_attn.fn.fn.to_qkv.weight" (3 heads 32, d)   "...fn.fn.to_out.weight"
 *   "init_temporal_attn.fn.fn.rotary_emb.freqs" (nrot; every module holds the same; not read when nrot = 0)
 *   "seqTransDecoder.decoder_layers.L.<self_attn.to_qkv.weight|self_attn.to_out.weight|multihead_attn.to_q.weight|
 *    multihead_attn.to_out.weight|ffn.linear1.weight|ffn.linear1.bias|ffn.linear2.weight|ffn.linear2.bias|layer_norm{1,2,3}.weight|bias>"
 * and three tables built at pack time (ctx.pbnet_named_weights):
 *   "bias_tgt.rel" "bias_mem.rel" (heads, 2 win + 1)  the relative-position bias of rel = key - query at [h][rel + win]
 *   "mem_kv.w" (n_layers * 2 * heads 32, d)            [to_k ; to_v] of every layer's multihead_attn one after the other: the decoder
 *                                                      memory is projected to all of them in one dawn_linear
 * Only pointers travel, so the shapes are the caller's to guarantee (ctx.pbnet_named_weights checks them). */
typedef struct dawn_pbnet dawn_pbnet;
typedef struct dawn_pbnet_cfg {
    int in_dim;                          /* pose 6 / blink 2 */
    int audio_dim;                       /* 1024 */
    int latent_dim;                      /* 256: width of z and of the audio embedding */
    int d;                               /* model width (64) */
    int heads;                           /* 4, of 32 */
    int ff;                              /* FFN width (1024) */
    int n_layers;                        /* decoder layers (4) */
    int win;                             /* eval-mode attention window in frames: 100 (transformerreemb6) / 200 (transformerreemb5) */
    int nrot;                            /* rotary pairs per head (2), at most 16 */
    float eps;                           /* LayerNorm eps (1e-5) */
} dawn_pbnet_cfg;
/* a missing name (named in the message), nrot > 16, or a width that is not positive: error return with a message, *out untouched */
int dawn_pbnet_create(const dawn_pbnet_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_pbnet** out);
void dawn_pbnet_destroy(dawn_pbnet* pb);
/* host code, exactly linear in T: a header of d floats rounded up to 256 bytes, then T rows each of (widths rounded up to 4 floats)
 *   d + 2 latent_dim  ztimelinear input [x_ref | z | audio embedding]      d  decoder memory      n_layers * 2 * heads 32  all layers' K | V
 *   3 x d  residual stream and two temporaries      3 heads 32  self-attention q | k | v      heads 32  cross-attention q
 *   heads 32  attention output      ff  FFN hidden      2 x nrot  rotary cos / sin
 * = 3,528 floats = 14,112 bytes per frame at the shipped widths.  0 for T < 1 or a NULL handle. */
size_t dawn_pbnet_workspace_bytes(const dawn_pbnet* pb, long T);
/* Decoder.forward for one sample: x0 (in_dim) first pose, audio (T, audio_dim) rows ld_audio apart, z (T, latent_dim) dense, all on the
 * device -> out (T, in_dim) rows ld_out apart.  T < 1, a NULL pointer, ld_audio < audio_dim, ld_out < in_dim, a short workspace or `out`
 * overlapping the workspace: error return with a message, nothing launched. */
int dawn_pbnet_generate(dawn_pbnet* pb, const float* x0, const float* audio, int ld_audio, const float* z, long T, float* out, int ld_out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* VideoGenerator.generate_pose_blink between its file reads and writes (UVG:252-302): init_pose6 / init_blink2 = the first 6 / 2 values
 * of the rows of init_pose.npy / init_eye_bbox.npy in HOST memory; the pose row is min-max normalised with (-90, -90, -90, 0, 0, 0) /
 * (90, 90, 90, 1, 720, 1080), both decoders run (pose: in_dim 6, blink: in_dim 2, latents z_pose / z_blink (T, latent_dim)), and
 * dri_pose = (out + ip) * (max - min) + min (every operation rounded on its own), dri_blink = out + ib, written at the caller's strides
 * ld_pose >= 6 / ld_blink >= 2 (other columns untouched).  Workspace: dawn_pose_blink_workspace_bytes = 256 bytes + the larger of the
 * two decoders' workspaces.  Refusals as dawn_pbnet_generate. */
size_t dawn_pose_blink_workspace_bytes(const dawn_pbnet* pose, const dawn_pbnet* blink, long T);
int dawn_pose_blink_stage(dawn_pbnet* pose, dawn_pbnet* blink, const float* audio, int ld_audio, long T, const float* init_pose6,
                          const float* init_blink2, const float* z_pose, const float* z_blink, float* dri_pose, int ld_pose,
                          float* dri_blink, int ld_blink, void* workspace, size_t workspace_bytes, void* stream);
/* ---- the clip inputs of FlowDiffusion.sample_one_video (FD:327-350) that no other stage makes (csrc/clip_inputs.hip): the 16
 * face-location channels of fea272 and the condition rows.  Once per clip, plain fp32, fixed summation order (bit-identical run to run).
 * FD:182-201 + FD:39-50.  bbox6 = HOST floats [x_min, x_max, y_min, y_max, H_src, W_src] (one sample); size = the square image side
 * (multiple of 4); w1 (8,1,3,3) b1 (8) w2 (16,8,3,3) b2 (16): the state_dict tensors as they are, on the device;
 * out = 16 planes of (size/4, size/4), `plane` floats apart (so it can be rows 256..271 of fea272).
 * The rectangle (FlowDiffusion.generate_bbox_mask, FD:187-193) is host arithmetic in fp32, every operation rounded on its own:
 * b[0:2] = b[0:2] / b[4] * size, b[2:4] = b[2:4] / b[5] * size, lt = trunc(b[0]), trunc(b[2]), rb = trunc(b[1] + 1), trunc(b[3] + 1),
 * truncation toward zero; a pixel is 1 where lt_y <= row <= rb_y and lt_x <= col <= rb_x (bounds outside the image are no error).
 * The kernel takes the four ints by value and evaluates the mask analytically: mask, conv1 (3x3 / stride 2 / pad 1) + ReLU and conv2
 * (the same) + ReLU in ONE launch, no mask and no intermediate tensor in memory; both convolutions pad with zeros; sums in the order
 * (channel, ky, kx).  size < 4 or size % 4 != 0, a NULL pointer, plane < (size/4)^2, a non-finite bbox6 or bbox6[4] / bbox6[5] == 0:
 * error return with a message, nothing launched. */
int dawn_face_loc_embed(const float* bbox6, int size, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* out, long plane, void* stream);
/* the four mask bounds alone, host code, for bindings and tests: lt_x, lt_y, rb_x, rb_y */
int dawn_bbox_mask_bounds(const float* bbox6, int size, int* bounds4);
/* FD:332-350.  audio (T, n_aud) rows ld_audio apart; pose (T, n_pose) rows ld_pose apart; eye (T, 2) rows ld_eye apart; all device.
 * init_pose = n_init HOST floats or NULL (n_init = 0: row 0 of `pose`); init_eye = 2 HOST floats or NULL (row 0 of `eye`).
 * P = n_init if init_pose else n_pose; n_pose must be P or P - 1 (then column P - 1 of the pose is init_pose[P - 1], FD:348-349).
 * cond (T, n_aud + P + 2) rows ld_cond apart = [audio | pose - init_pose | eye - init_eye], each a single fp32 subtraction.
 * Each input may be exactly the columns of `cond` it lands in (same address, ld == ld_cond: what dawn_hubert_features /
 * dawn_pose_blink_stage leave when they wrote into `cond`; audio columns are then not touched at all); otherwise it must not overlap
 * `cond`.  With a NULL init the rows after the first go in one launch and row 0 in a second one, so that in place no row reads a
 * row 0 that was overwritten.  T < 1, a NULL pointer, a stride smaller than its width, n_pose not in {P, P - 1}, n_init > 16,
 * non-finite host init values, any other overlap: error return with a message, nothing launched. */
int dawn_cond_rows(const float* audio, int n_aud, int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye, int ld_eye,
                   const float* init_pose, int n_init, const float* init_eye, long T, float* cond, int ld_cond, void* stream);
/* ---- the same as a stage host (csrc/dawn_inputs.hip), the fifth beside dawn_ctx / dawn_decoder / dawn_hubert / dawn_pbnet and with
 * their contract: opaque handle, device pointers by name, every launch on `stream`, no allocation, no synchronisation; an error return
 * comes with a dawn_last_error message and nothing launched.  Weight names = FlowDiffusion's own state_dict keys:
 *   "face_loc_emb.conv1.weight" (8,1,3,3)  "face_loc_emb.conv1.bias" (8)  "face_loc_emb.conv2.weight" (16,8,3,3)  "face_loc_emb.conv2.bias" (16)
 * Reference quirk, kept: the reference never saves face_loc_emb (video_generator.py:58 stores the unet and the diffusion only), so no
 * checkpoint holds these four tensors; the host supplies whatever its FlowDiffusion holds. */
typedef struct dawn_inputs dawn_inputs;
typedef struct dawn_inputs_cfg { int n_aud; int pose_dim; int eye_dim; } dawn_inputs_cfg;     /* 1024, 6 or 7, 2 */
int  dawn_inputs_create(const dawn_inputs_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_inputs** out);
void dawn_inputs_destroy(dawn_inputs* in);
/* fea272 rows fea_ch - 16 .. fea_ch - 1 (256..271) from the bbox (dawn_face_loc_embed), and the cond rows (dawn_cond_rows with n_aud
 * and P = pose_dim of the handle); fea272 = (fea_ch, size/4, size/4), whose first fea_ch - 16 planes dawn_decoder_encode writes.  Both
 * calls are checked before the first launch. */
int  dawn_clip_inputs(dawn_inputs* in, const float* bbox6, int size, float* fea272, int fea_ch,
                      const float* audio, int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye, int ld_eye,
                      const float* init_pose, int n_init, const float* init_eye, long T, float* cond, int ld_cond, void* stream);
/* ---- one call from 16 kHz samples and a source image to frame bytes (VideoGenerator.generate UVG:304-399 without its files), built
 * only from the entry points above, in this order: dawn_hubert_features -> two dawn_philox_normal draws (z_pose, z_blink) ->
 * dawn_pose_blink_stage into the pose / eye columns of cond -> dawn_decoder_encode (fea_out = planes 0 .. fea_ch - 17 of fea272) ->
 * dawn_clip_inputs in place on cond -> dawn_clip_prepare (and the null clip when cond_scale != 1) -> dawn_philox_normal (x_init) ->
 * dawn_sampler_run_clip / dawn_sampler_run_ancestral_clip -> dawn_decode_clip / dawn_decode_clip_yuv420.
 * Random draws, so that a host running the stages itself gets the same bits: x_init = dawn_philox_normal(3, T, 0, T, h w, seed, stream
 * id 0); the sampler's steps use stream ids from 1 (dawn_sampler_run); z_pose = (1, T, 0, T, latent_dim, seed, 0xFFFFFFFE) and z_blink
 * the same with 0xFFFFFFFF: (1, T, latent_dim) each.
 * T is the caller's: min(max_n_frames, num_frames) as UVG:329 with num_frames from dawn_hubert_segments; T above num_frames is refused.
 * All pointers are device pointers except the ones marked HOST.  The five handles must belong together (the caller's to guarantee:
 * only pointers travel): hubert hidden = pbnet audio_dim = inputs n_aud; unet cond columns = [n_aud | pose_dim | 2], unet fea_ch =
 * decoder bottleneck width + 16; decoder n_down = 2 (h = w = H / 4). */
enum { DAWN_FRAMES_RGB = 0, DAWN_FRAMES_YUV420 = 1 };
typedef struct dawn_generate_args {
    dawn_hubert* hubert; dawn_pbnet* pose; dawn_pbnet* blink; dawn_decoder* decoder; dawn_inputs* inputs; dawn_ctx* unet;
    const float* samples; long n_samples;            /* raw fp32 16 kHz samples */
    const float* img3; int H;                        /* source image (3, H, H) planar in [0, 1] */
    int fea_ch;                                      /* the unet's fea_ch (272) */
    const float* bbox6;                              /* HOST, as dawn_face_loc_embed */
    const float* init_pose; const float* init_eye;   /* HOST or NULL, as dawn_cond_rows (n_init values / 2 values) */
    int n_init;
    int latent_dim;                                  /* the PBnets' latent width (256), a multiple of 4 */
    const float* init_pose6; const float* init_blink2;   /* HOST, as dawn_pose_blink_stage */
    long T; int S;                                   /* frames; sampler steps */
    float cond_scale;
    const dawn_ddim_step* ddim_steps;                /* HOST, S entries: DDIM -- or */
    const dawn_ancestral_step* ancestral_steps;      /* HOST, S entries: ancestral; exactly one of the two tables */
    const dawn_clip_mode* clip;                      /* HOST or NULL = {DAWN_CLIP_DYNAMIC, 0.9} */
    uint64_t seed;
    int format; int bgr; int chunk;                  /* DAWN_FRAMES_*; bgr: RGB frames only; frames decoded `chunk` at a time */
    const double* mean3;                             /* HOST or NULL, as dawn_decode_clip */
    unsigned char* frames_out;                       /* (T,H,H,3) or (T, 3 H H / 2) uint8: clip_bytes of dawn_generate_bytes */
    float* latent_out;                               /* optional (3,T,h,w): the sampler's latent */
    float* cond_out;                                 /* optional (T, n_aud + pose_dim + 2) dense: the condition rows */
} dawn_generate_args;
/* host code: *clip_bytes = the bytes of frames_out, *workspace_bytes = cond, a zero row (guided), fea272, the audio rows, z_pose /
 * z_blink, x_init and the latent, the decoder skips, the clip tables (twice when guided) -- each rounded up to 256 bytes; cond and the
 * latent only where cond_out / latent_out are NULL -- plus the LARGEST of the stages' own workspaces (the stages run one after the
 * other).  An argument dawn_generate_clip would refuse: the same error return, both sizes untouched. */
int dawn_generate_bytes(const dawn_generate_args* args, size_t* clip_bytes, size_t* workspace_bytes);
/* every argument is checked before the first launch: a refusal (NULL handle or pointer, T above what the audio yields, a short
 * workspace, ...) comes with a message and nothing launched.  latent_out / cond_out / frames_out must not overlap the workspace. */
int dawn_generate_clip(const dawn_generate_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* ---- media ingest (csrc/media_ingest.hip): from what a host holds after decoding to what dawn_generate_clip takes.  Contract as the
 * stage entry points: every launch on `stream`, no allocation, no synchronisation, every argument checked before the first launch; a
 * refusal returns non-zero with a dawn_last_error message that names the argument, and launches nothing.
 * UVG:320-325 (Image.open(...).convert("RGB") -> transforms.Resize((size, size)) -> ToTensor()): Pillow's 8-bit antialiased bilinear
 * resample, restated in integers and bit-identical to it.  src = Hs rows of Ws interleaved pixels, device bytes, rows row_bytes >=
 * Ws * pix_bytes apart, no alignment asked of the pointer or of row_bytes.  pix_bytes 1 = grey, replicated to the three planes as
 * .convert("RGB") does for mode "L"; 3 = RGB / BGR; 4 = the same with a fourth byte that is never read (.convert("RGB") drops alpha).
 * order = DAWN_PIXELS_RGB / DAWN_PIXELS_BGR (ignored for pix_bytes 1).  out3 = three planes of Ho * Wo floats, `plane` floats apart,
 * in R, G, B order whatever `order` is; a value = (float)byte / 255.0f, one correctly rounded fp32 division (= ToTensor()'s value, and
 * for all 256 bytes = (ToTensor(x) * 255) / 255. as the generator forms it).
 * Per axis with input length n and output length m, in fp64 with every operation rounded on its own (no fused multiply-add):
 *   scale = n / m; fs = max(scale, 1); support = fs; ss = 1 / fs
 *   center = (i + 0.5) * scale; lo = max((int)(center - support + 0.5), 0); hi = min((int)(center + support + 0.5), n)
 *   w[j] = max(1 - |(j + lo - center + 0.5) * ss|, 0), j < hi - lo; ww = w[0] + w[1] + ... left to right
 *   k[j] = (int)(0.5 + (w[j] / ww) * 4194304.0); out = clip to 0..255 of ((1 << 21) + sum_j in[lo + j] * k[j]) >> 22, the sum in int32
 * (Pillow's precompute_coeffs with the bilinear filter and normalize_coeffs_8bpc; the tables are made on the device).
 * PASS ORDER: the horizontal pass (Ws -> Wo) runs first and stores BYTES, the vertical pass runs on those bytes -- always.  A pass whose
 * input and output lengths are equal is skipped, not run with unit weights; with both skipped the call is the layout conversion and the
 * division alone.  The horizontal pass touches only the source rows that a vertical tap reads.  Horizontal-first is the classic Pillow
 * order; Pillow 12.2.0 was seen to run the vertical pass first on some tall and narrow shapes (1023 x 3 -> 8 x 8, 4000 x 6 -> 4 x 4) and
 * then differs from this entry point by one level, while it agrees bit for bit on 2160 x 3840 -> 8 x 8, 1080 x 1920 -> 12 x 12,
 * 777 x 1333 -> 8 x 16, 257 x 255 -> 256 x 256 and small shapes of every kind (tests/ingest_cases.py).
 * The source is read through aligned 32-bit loads: up to three bytes in front of a row and behind it are fetched (bytes of an aligned word
 * that also holds a byte of the row) and never used.
 * Refused: a NULL pointer, a side below 1 or above 65535, pix_bytes not in {1, 3, 4}, an unknown order, row_bytes < Ws * pix_bytes,
 * plane < Ho * Wo, a workspace below dawn_image_ingest_workspace_bytes (the message states both sizes), out3 overlapping the workspace. */
enum { DAWN_PIXELS_RGB = 0, DAWN_PIXELS_BGR = 1 };
/* host code: both coefficient tables with their (lo, taps) pairs and the byte image between the two passes, each piece rounded up to 256
 * bytes and sized whether or not its pass runs, so that the size grows with every argument; 0 for a side outside 1 .. 65535 */
size_t dawn_image_ingest_workspace_bytes(int Hs, int Ws, int Ho, int Wo);
int dawn_image_ingest(const unsigned char* src, int Hs, int Ws, long row_bytes, int pix_bytes, int order, int Ho, int Wo, float* out3,
                      long plane, void* workspace, size_t workspace_bytes, void* stream);
/* UVG:226, 451-452 (soundfile.read, then speech[:, 0]): out[i] = (float)pcm[i * channels] / 32768.0f for i < n_frames -- channel 0 of
 * interleaved 16-bit PCM with soundfile's int16 scaling, exact in fp32.  pcm needs 2-byte alignment only.  Refused: a NULL or odd
 * pointer, n_frames < 1, channels outside 1 .. 8. */
int dawn_pcm16_to_samples(const int16_t* pcm, long n_frames, int channels, float* out, void* stream);
/* ---- dawn_generate_clip from decoded media: the two conversions above, then the pipeline.  `gen` is a HOST struct filled as for
 * dawn_generate_clip; with `image` set its img3 is ignored and the image is ingested to (3, gen->H, gen->H); with `pcm` set its samples /
 * n_samples are ignored and channel 0 of the n_frames PCM frames is the audio (T above what n_frames yields is refused exactly as there).
 * A NULL image / pcm keeps gen->img3 / gen->samples; with both NULL the call IS dawn_generate_clip.  The workspace holds, in front of
 * what dawn_generate_bytes asks for, img3 (3 H H floats), the fp32 samples and the ingest workspace -- each rounded up to 256 bytes and
 * only for the input that is given: dawn_generate_media_bytes is dawn_generate_bytes plus those pieces.  Everything is checked before the
 * first launch: what dawn_generate_clip, dawn_image_ingest and dawn_pcm16_to_samples refuse is refused here, under this entry's name. */
typedef struct dawn_media_args {
    const dawn_generate_args* gen;     /* HOST; its img3 / samples / n_samples are ignored when the fields below replace them */
    const unsigned char* image; int Hs, Ws; long row_bytes; int pix_bytes, order;   /* NULL image: gen->img3 is used */
    const int16_t* pcm; long n_frames; int channels;                                /* NULL pcm: gen->samples is used */
} dawn_media_args;
int dawn_generate_media_bytes(const dawn_media_args* args, size_t* clip_bytes, size_t* workspace_bytes);
int dawn_generate_clip_media(const dawn_media_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* ---- audio at any sample rate (csrc/audio_resample.hip): resample to the 16 kHz mono fp32 samples that the HuBERT stage takes.  It stands
 * where the reference runs `ffmpeg -ar 16000` (UVG:223, 416-431), but its values are THIS definition's, not ffmpeg's: swresample's output
 * depends on build and version, bit parity with it is not a goal, and nobody has measured what the difference does to the HuBERT features.
 * Contract as the media ingest above (every launch on `stream`, no allocation, no synchronisation, everything checked before the first launch).
 * Z = 32 (zero crossings per side), BETA = 9.0 (Kaiser), CUT = 0.92.  For an integer `rate`, 1000 <= rate <= 384000, rate != 16000:
 *   g = gcd(16000, rate); L = 16000 / g; M = rate / g; n_out = floor(n_frames * 16000 / rate) in 64-bit integers (n_out < 1 is refused)
 *   rho = 1 if rate <= 16000, else 16000.0 / rate; W = Z / rho is the half width in input samples (fp64); K = ceil(W)
 *   h(u) = rho * CUT * sinc(rho * CUT * u) * I0(BETA * sqrt(1 - (u / W)^2)) / I0(BETA) for |u| < W, and 0 otherwise
 *   sinc(t) = sin(pi t) / (pi t), sinc(0) = 1; I0(x) = sum_k ((x / 2)^k / k!)^2, summed until a term falls below 2^-60 of the sum
 *   coef[r][j + K] = h(r / L - j) for r = 0 .. L - 1, j = -K .. K: L rows of 2 K + 1 fp64 values, made on the device in the workspace
 *   for output i: (q, r) = divmod(i * M, L) in 64-bit integers; y[i] = sum_{j = -K .. K} x[q + j] * coef[r][j + K], j ascending
 * with x[k] = 0 outside 0 <= k < n_frames, x exact (channel 0 of the PCM / 32768, or the fp32 sample), the sum in fp64 and ONE rounding to
 * fp32; no clipping, |y| may exceed 1.  The position q + r / L is never formed as one floating-point number.  Bit-identical run to run.
 * rate == 16000 is not filtered: the PCM entry is dawn_pcm16_to_samples bit for bit, the fp32 entry a copy, and no workspace is needed
 * (it may be NULL; dawn_resample16k_workspace_bytes(16000) = 0).  The PCM pointer needs 2-byte alignment only; x and out 4-byte, the
 * workspace 8-byte.  n_frames is at most 2^34.
 * Refused, with a message that names the argument and nothing launched: a NULL or misaligned pointer, channels outside 1 .. 8, rate outside
 * 1000 .. 384000, n_frames < 1, n_out != dawn_resample16k_len(n_frames, rate) (the message states both), n_out < 1, a workspace below
 * dawn_resample16k_workspace_bytes(rate) (the message states both sizes), out overlapping the workspace. */
long dawn_resample16k_len(long n_frames, int rate);            /* host: n_out; 0 where the call would be refused */
size_t dawn_resample16k_workspace_bytes(int rate);             /* host: the table, rounded up to 256 bytes; 0 for a rate outside the range (and for 16000) */
int dawn_resample16k_pcm16(const int16_t* pcm, long n_frames, int channels, int rate, float* out, long n_out, void* workspace,
                           size_t workspace_bytes, void* stream);
int dawn_resample16k_f32(const float* x, long n_frames, int rate, float* out, long n_out, void* workspace, size_t workspace_bytes,
                         void* stream);
/* dawn_generate_clip_media with PCM at `pcm_rate`: the PCM goes through dawn_resample16k_pcm16, whose n_out samples and table are carved
 * from the front of the workspace with the other pieces (dawn_generate_media_rate_bytes counts them); "T above what the audio yields" is
 * judged on n_out.  pcm_rate == 16000 IS dawn_generate_clip_media: the same launches, the same bits, the same sizes.  A NULL pcm with
 * pcm_rate != 16000 is refused (gen->samples are 16 kHz samples already); what dawn_resample16k_pcm16 refuses is refused here, under this
 * entry's name, before the first launch.  The rate is a parameter, not a field: dawn_media_args is unchanged. */
int dawn_generate_media_rate_bytes(const dawn_media_args* args, int pcm_rate, size_t* clip_bytes, size_t* workspace_bytes);
int dawn_generate_clip_media_rate(const dawn_media_args* args, int pcm_rate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LFG motion encode, batched over the frames of a driving video (csrc/motion_encode.hip) -------------------------
 * The encode half of the frozen LFG (FD:248-262): RegionPredictor (RP = LFG/modules/region_predictor.py), BGMotionPredictor (BG =
 * bg_motion_predictor.py) and Generator.forward's PixelwiseFlowPredictor (PF = pixelwise_flow_predictor.py; UTIL = util.py), for the
 * shipped configuration (pca_based, estimate_affine, revert_axis_swap, bg_type 'affine', use_deformed_source, use_covar_heatmap,
 * estimate_occlusion_map).  The five entries below are everything that is not a convolution; the three conv stacks between them run on
 * dawn_conv_gemm / dawn_affine_act / dawn_bn_relu_pool2 (dawn_pytorch_amd/motion_encoder.py).  Activations are channels-last rows.
 * Stage contract: every launch on `stream`, no allocation, no synchronisation, every argument checked before the first launch, a refusal
 * names the argument.  The coordinate grid is make_coordinate_grid's (UTIL:51-67), fp32, each operation rounded on its own:
 *     g(j, n) = 2 * (j / (n - 1)) - 1        x: j = column, n = w;  y: j = row, n = h        (so h, w >= 2) */
/* AntiAliasInterpolation2d (UTIL:217-264) at scale 1 / s, s = 1 .. 8 (s = 1: one tap of weight 1, the layout change alone), only the kept pixels: with sigma = (s - 1) / 2, K = 4 (s - 1) + 1
 * taps (= 2 round(4 sigma) + 1: sigma 1.5 and 13 taps at s = 4), ka = K / 2 and g[i] = fp32(exp(-(i - ka)^2 / (2 sigma^2))),
 *     out[t][yo][xo][c] = ( sum_i g[i] * ( sum_j g[j] * in[t][c][s yo - ka + i][s xo - ka + j] ) ) / S,     S = fp32 sum_ij fp32(g[i] g[j]),
 * taps outside the H x W frame read zero (the reference's F.pad), sums in fp32 with fused multiply-adds, j inside i; ho = ceil(H / s),
 * wo = ceil(W / s).  This is the reference's fp32 product kernel divided by its fp32 sum, factored.
 * in_kind 0: fp32 planes, in[t][c][y][x] at in + t * frame_stride + c * chan_stride + y * W + x floats (both (T,3,H,W) and (3,T,H,W));
 * in_kind 1: uint8 frames (T,H,W,3) as ingest and egress make them, frame t at in + t * frame_stride bytes, value = byte / 255.
 * out: rows (T * ho * wo, ld_out) as dawn_conv_gemm reads them: channels 0 .. 2 the result, channels 3 .. c_pad - 1 written as zero. */
int dawn_antialias_down(const void* in, int in_kind, long frame_stride, long chan_stride, int T, int H, int W, int s, float* out, int ld_out,
                        int c_pad, void* stream);
/* RegionPredictor after its `regions` conv (RP:84-117, RP:60-75), per frame t and region r, from x (T, h * w, R) with row stride ld:
 *     e[p]   = exp((x[t][p][r] - max_p x[t][p][r]) / temperature)                      fp64
 *     shift  = sum_p e[p] g[p] / sum_p e[p],    covar = sum_p e[p] g[p] g[p]^T / sum_p e[p] - shift shift^T        fp64 sums, fp32 results
 *     affine = U diag(sqrt(s1), sqrt(s2)),  covar = U diag(s1, s2) U^T, s1 >= s2 >= 0, in closed form from the fp64 covar = [[a, b], [b, c]]:
 *              hd = (a - c) / 2, rad = sqrt(hd^2 + b^2), s1 = (a + c) / 2 + rad, s2 = max((a c - b^2) / s1, 0);
 *              u1 = the unit vector along (hd + rad, b) where hd >= 0, along (b, rad - hd) otherwise, (1, 0) where that vanishes;
 * SIGN CONVENTION: u1.x > 0, or u1.x == 0 and u1.y > 0;  u2 = (u1.y, -u1.x), so det U = -1 always (torch.svd's U of such matrices has
 * det -1 too except on exactly diagonal input; only A_s . inverse(A_d) is used downstream, and after revert_axis_swap's sign(M[0][0]) that
 * product is the same for every convention with a fixed det U).  The heatmap (T, R, h, w) is never written: nothing at inference reads it.
 * shift (T, R, 2) = (x, y);  covar, affine (T, R, 2, 2) row-major. */
int dawn_region_moments(const float* x, int ld, int T, int h, int w, int R, double temperature, float* shift, float* covar, float* affine,
                        void* stream);
/* BGMotionPredictor after its encoder (BG:46-52, bg_type 'affine'): x (T, npix, C) with row stride ld = the encoder's last map,
 *     v[o] = fc_b[o] + sum_c fc_w[o][c] * (sum_p x[t][p][c] / npix),  o = 0 .. 5     (fp64 sums, rounded once)
 *     out[t] = [[v0, v1, v2], [v3, v4, v5], [0, 0, 1]]                                (T, 3, 3) */
int dawn_bg_params(const float* x, int ld, int T, int npix, int C, const float* fc_w, const float* fc_b, float* out, void* stream);
/* The pixelwise hourglass's input rows (PF:48-120), written directly: out (T * h * w, ld_out), channel 4 k + j of pixel p of frame t,
 * k = 0 .. R (0 = background), from the per-frame driving parameters drv_* (T, R, ...), the per-clip source parameters src_* (R, ...),
 * bg_params (T, 3, 3) and the downsampled source src_rows (h * w, ld_src), 3 channels:
 *     motion_0 = (X / Z, Y / Z), (X, Y, Z) = bg[t] . (gx, gy, 1)
 *     motion_k = M_k . (g - shift_d,k) + shift_s,k,   M_k = A_s,k . inverse(A_d,k),  M_k *= sign(M_k[0][0])   (sign(0) = 0)
 *     j = 0:      k = 0: 0;  k >= 1: gauss(g; shift_d,k, covar_d,k) - gauss(g; shift_s,k, covar_s,k),  gauss = exp(-(d^T C^-1 d) / 2), d = g - shift
 *     j = 1 .. 3: grid_sample(source, motion_k) -- bilinear, zeros, align_corners=False (dawn_warp_blend's corner set) -- channel j - 1
 * M_k and the inverse covariances: fp64, closed-form 2x2 inverses, rounded to fp32; everything per pixel: fp32.  Channels 4 (R + 1) ..
 * c_pad - 1 are written as zero (c_pad % 4 == 0, <= 64; ld_out % 4 == 0; out 16-byte aligned).  Neither the R + 1 motion grids nor the
 * R + 1 warped images are stored. */
int dawn_motion_inputs(const float* drv_shift, const float* drv_covar, const float* drv_affine, const float* src_shift, const float* src_covar,
                       const float* src_affine, const float* bg_params, int R, const float* src_rows, int ld_src, int T, int h, int w,
                       float* out, int ld_out, int c_pad, void* stream);
/* PF:124-135 on x (T * h * w, ld): channels 0 .. R the `mask` conv, channel R + 1 the `occlusion` conv (run as one 7x7 conv):
 *     m = softmax(x[0 .. R]);   flow = sum_k m[k] * motion_k  (k ascending, the motions of dawn_motion_inputs recomputed);   occ = sigmoid(x[R + 1])
 * grid: the x plane of frame t at grid + t * h * w, the y plane grid_plane floats further ((2, T, h, w) slices of the latent);
 * conf + t * h * w receives occ, or with conf_x0 = 1 the diffusion's x0 plane 2 * occ - 1 (FD:274-282). */
int dawn_flow_combine(const float* x, int ld, const float* drv_shift, const float* drv_affine, const float* src_shift, const float* src_affine,
                      const float* bg_params, int R, int T, int h, int w, float* grid, long grid_plane, float* conf, int conf_x0, void* stream);
/* ---- SURVEY 8(f) N5 as a whole path: the motion-encode stage from a source image and driving frames to the flow / occlusion latent
 * (csrc/dawn_motion.hip).  The launch sequence of dawn_pytorch_amd/motion_encoder.py (MotionEncoder._encode) through the per-op entries
 * of this library with the same arguments -- dawn_antialias_down, dawn_conv_gemm, dawn_bn_relu_pool2, dawn_affine_act,
 * dawn_region_moments, dawn_bg_params, dawn_motion_inputs, dawn_flow_combine -- so the bits are those of the Python orchestration.  The
 * one launch Python does not have: the source half of the background encoder's first conv, which Python repeats per chunk with
 * expand().reshape(), is repeated by a copy kernel here (no arithmetic).  Same contract as dawn_decoder: opaque handle, device pointers
 * by name, caller-owned workspace, every launch on `stream`, no allocation, no synchronisation; an error return comes with a
 * dawn_last_error message and nothing launched.  The handle is immutable after creation.  One clip per call (B = 1).
 * Weight names = ctx.motion_named_weights(encoder), from the packed _Conv images of MotionEncoder (pack.py and motion_encoder.py stay
 * the one definition of the layouts and of the zero padding of every channel count to a multiple of 16).  <conv> = "w" (pack_kn image;
 * an up block: the four phase images), "ws" (pack_bf3 image, 3x3 convs), "bias"; "a" "b" = the BatchNorm that follows, as scale / shift:
 *   "rp.down.i.<conv>" "rp.down.i.a|b"   "rp.up.i.<conv>" "rp.up.i.a|b"   "rp.regions.w" "rp.regions.bias"      region predictor
 *   "bg.src0.<conv>"   "bg.drv0.w" "bg.drv0.ws"   "bg.down.0.a|b"   "bg.down.i.<conv>" "bg.down.i.a|b" (i >= 1)   "fc.w" "fc.b"
 *                                                    background encoder, its first conv as a source half (with the bias) and a driving half
 *   "pf.down.i.<conv>" "pf.down.i.a|b"   "pf.up.i.<conv>" "pf.up.i.a|b"   "pf.out.w" "pf.out.bias"              pixelwise flow predictor
 *                                                    ("pf.out" = the mask and occlusion convs as one 7x7 conv of R + 2 outputs) */
#define DAWN_MOTION_MAX_BLOCKS 8
typedef struct dawn_motion dawn_motion;
typedef struct dawn_motion_cfg {
    int R;                                   /* regions, 1 .. 15 (10) */
    int s;                                   /* 1 / scale_factor of both predictors, 1 .. 8 (4): the latent is ceil(H / s) x ceil(W / s) */
    double temperature;                      /* RegionPredictor's softmax temperature (0.1), the double dawn_region_moments takes */
    int rp_blocks, bg_blocks, pf_blocks;     /* down blocks of the region hourglass (= its up blocks), of the background encoder, of the
                                                pixelwise hourglass: 1 .. DAWN_MOTION_MAX_BLOCKS each, refused beyond */
    int rp_down[DAWN_MOTION_MAX_BLOCKS], rp_up[DAWN_MOTION_MAX_BLOCKS];     /* REAL (unpadded) output channels of every block; the */
    int bg_down[DAWN_MOTION_MAX_BLOCKS];                                    /* buffers hold each rounded up to a multiple of 16.  The */
    int pf_down[DAWN_MOTION_MAX_BLOCKS], pf_up[DAWN_MOTION_MAX_BLOCKS];     /* hourglass inputs are 3 and 4 (R + 1) channels */
} dawn_motion_cfg;
/* a missing name, a count outside its range: error return with a message that names it, *out untouched */
int dawn_motion_create(const dawn_motion_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_motion** out);
void dawn_motion_destroy(dawn_motion* m);
/* host code: bytes of the workspace for H x W frames encoded `chunk` frames at a time (1 .. 4096) -- independent of the clip length:
 * the per-clip source pieces, a chunk's activations and, so that driving kind 2 needs no more, a chunk of RGB bytes.  0 (with a
 * message) for sizes the stage refuses. */
size_t dawn_motion_workspace_bytes(const dawn_motion* m, int H, int W, int chunk);
/* src = ONE H x W image, drv = T frames of that size.  Kinds as dawn_antialias_down: 0 = fp32 planes (src: channel c at src + c * H * W
 * floats; drv: frame t, channel c at drv + t * drv_frame_stride + c * drv_chan_stride floats, so (T,3,H,W) and (3,T,H,W) both go),
 * 1 = uint8 RGB frames (frame t at drv + t * drv_frame_stride bytes, drv_frame_stride >= 3 H W; drv_chan_stride ignored); driving kind
 * 2 = I420 frames as dawn_yuv420_to_frames takes them (frame t at drv + t * drv_frame_stride bytes, >= 3 H W / 2), converted chunk by
 * chunk into the workspace with that kernel and then read as kind 1: a full-clip RGB copy never exists.  src kind 2 is refused.
 * The source work happens once, first (its downsampled image, its region parameters, its half of the background encoder's first
 * conv); then the frames go `chunk` at a time (a ragged last chunk is fine; chunk above T counts as T).
 * Outputs = dawn_flow_combine's: the x plane of frame t at grid + t * h * w, the y plane grid_plane floats further (grid_plane >= T h w),
 * conf (T,h,w) the occlusion map -- or 2 * conf - 1 with conf_x0 = 1 (the diffusion's x0 plane); h = ceil(H / s), w = ceil(W / s).
 * Refused before the first launch, the cause named: a NULL argument, T < 1, chunk < 1, an unknown kind, H or W not divisible by
 * 2^bg_blocks, h or w not divisible by 2^rp_blocks and 2^pf_blocks (or below 2), short strides, a workspace below
 * dawn_motion_workspace_bytes(m, H, W, min(chunk, T)), an output that overlaps the workspace, and what dawn_yuv420_to_frames refuses. */
int dawn_motion_encode_clip(dawn_motion* m, int H, int W, int T, const void* src, int src_kind, const void* drv, int drv_kind,
                            long drv_frame_stride, long drv_chan_stride, int chunk, float* grid, long grid_plane, float* conf, int conf_x0,
                            void* workspace, size_t workspace_bytes, void* stream);
/* ---- video-driven reenactment in one call (FlowDiffusion.reenact): source image + driving frames -> frame bytes, built from
 * dawn_motion_encode_clip (into grid / conf) -> dawn_decoder_encode -> dawn_decode_clip_conf (DAWN_FRAMES_RGB) or
 * dawn_decode_clip_conf_yuv420 (DAWN_FRAMES_YUV420).  No UNet, no audio.  `size` = sizeof(dawn_reenact_args) of the caller's header:
 * another value is refused.  All pointers are device pointers except mean3. */
typedef struct dawn_reenact_args {
    size_t size;
    dawn_motion* motion; dawn_decoder* decoder;
    const float* img3; int H, W;                     /* source image (3,H,W) fp32 planar in [0,1]: both stages read it */
    const void* drv; int drv_kind; int T;            /* as dawn_motion_encode_clip */
    long drv_frame_stride, drv_chan_stride;
    int motion_chunk, chunk;                         /* frames per chunk of the encode / of the decode */
    int format, bgr;                                 /* DAWN_FRAMES_* as dawn_generate_args; bgr: RGB frames only */
    const double* mean3;                             /* HOST or NULL, as dawn_decode_clip */
    unsigned char* frames_out;                       /* (T,H,W,3) or (T, 3 H W / 2) uint8: clip_bytes of dawn_reenact_bytes */
    float* grid_out; float* conf_out;                /* optional, both or neither: (2,T,h,w) dense and (T,h,w), the encoded motion */
} dawn_reenact_args;
/* host code: *clip_bytes = the bytes of frames_out; *workspace_bytes = grid and conf (where grid_out / conf_out are NULL), the decoder's
 * skip memory -- each rounded up to 256 bytes -- plus the larger of the two stages' workspaces.  What dawn_reenact_clip would refuse:
 * the same error return, both sizes untouched. */
int dawn_reenact_bytes(const dawn_reenact_args* args, size_t* clip_bytes, size_t* workspace_bytes);
int dawn_reenact_clip(const dawn_reenact_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* ---- model bundle (csrc/dawn_bundle.hip, csrc/dawn_bundle_format.h): ONE file that holds everything the six *_create calls and
 * dawn_generate_args need besides the media -- the packed weight tables, the six cfg structs, named step tables and a defaults
 * record -- so that a host without Python runs the pipeline (tools/dawn_generate.cpp).  Python writes it (dawn_pytorch_amd/bundle.py:
 * the packers of pack.py / ctx.py stay the one definition of every packed layout; the loader copies bytes and never looks inside).
 * THE FORMAT, version 1.  Little-endian, every offset and size an unsigned 64-bit number, no compression, nothing optional.
 *   header, 64 bytes:   0 magic "DAWNBNDL"   8 u32 version = 1   12 u32 abi (dawn_abi_version() the struct blobs were written for)
 *                       16 u64 n_entries   24 u64 index_bytes   32 u64 payload_offset (multiple of 256, at or after the index end)
 *                       40 u64 device_bytes (multiple of 256)   48 u64 file_bytes (the whole file)   56 u64 zero
 *   index at byte 64, index_bytes long, n_entries entries back to back, each 48 bytes + the name:
 *                       0 u32 stage (DAWN_STAGE_*)   4 u32 kind (DAWN_BUNDLE_DEVICE / _HOST)   8 u32 dtype (informational: 0 bytes,
 *                       1 f32, 2 bf16, 3 f16, 4 i32, 5 f64, 6 i64, 7 i16)   12 u32 name_len (1 .. 4096)   16 u64 offset from the payload
 *                       start   24 u64 length in bytes   32 u64 s1   40 u64 s2   48 the name, zero-padded to a multiple of 8 bytes
 *   payload at payload_offset: first the device part, bytes [0, device_bytes), then the host part up to the end of the file.
 *     device tensor: offset a multiple of 256, length the tensor's bytes zero-padded to a multiple of 4 (a bf16 split image may hold an
 *                    odd element count), inside the device part; the bytes between tensors are zero.  The device part goes to the GPU
 *                    as one region and a tensor's pointer is base + offset.
 *     host blob:     offset a multiple of 16, inside the host part (at most 64 MiB).  "cfg" of a stage = the raw bytes of its cfg struct
 *                    (dawn_hubert_cfg, dawn_pbnet_cfg for pose and blink, dawn_decoder_cfg, dawn_inputs_cfg, dawn_unet_cfg); in the stage
 *                    DAWN_STAGE_HOST: "defaults" = one dawn_bundle_defaults, "steps.ddim.<S>" = S dawn_ddim_step,
 *                    "steps.ancestral.<S>" = S dawn_ancestral_step (written by sampler.ddim_step_scalars / ancestral_step_scalars:
 *                    the schedule arithmetic keeps its single definition); other names are the host's own.
 *   A length of 0, two entries that overlap, a name given twice within (stage, kind), a struct blob whose length is not its sizeof
 *   (a step table: not a multiple of it): refused.
 *   checksum of an entry: its bytes (a host blob zero-padded to whole words) as n little-endian 32-bit words w[0..n-1],
 *     s1 = sum w[i] mod 2^64, s2 = sum (i + 1) w[i] mod 2^64.  A flipped bit changes s1, two exchanged unequal words change s2.  It is an
 *     INTEGRITY check against truncated files, bad copies and stale bundles; it is NO protection against tampering.
 * THE LOADER.  dawn_bundle_open is host code (no GPU call): it reads and validates header, index and host part (host blobs are checked
 * against their checksums there) and refuses, with a message that names the field or the entry, everything the format forbids, an ABI
 * number other than dawn_abi_version() and a file whose size is not the header's; all offset arithmetic is overflow-checked.
 * dawn_bundle_upload copies the device part of the file into the caller's allocation (256-byte aligned, at least
 * dawn_bundle_device_bytes): the ONE entry that does file I/O, and it BLOCKS until the copy is done (it synchronises `stream`); its
 * staging memory is the library's own, two pinned buffers of 8 MiB whatever the file size.
 * dawn_bundle_verify checksums every device tensor ON THE DEVICE (so the copy is covered too): the host cuts the tensors into work
 * items (tensor, first word, at most 65536 words), ONE launch (per 2^20 items) writes one (s1, s2) pair per item into the workspace
 * [work list | partials] of dawn_bundle_verify_workspace_bytes, the host adds the pairs per tensor in exact 64-bit integers and compares
 * with the index.  Integer arithmetic only: the result does not depend on launch geometry or order.  It BLOCKS (it reads the pairs back)
 * and returns non-zero naming the first failing stage and tensor.  Both refuse a short allocation before touching anything.
 * dawn_bundle_table yields the dawn_named_ptr array of a stage for the region at device_mem, owned by the handle and valid until close
 * (or the next call for that stage); pass it straight to dawn_*_create.  dawn_bundle_cfg copies a stage's cfg struct (out_bytes must be
 * its sizeof); dawn_bundle_host returns a blob of DAWN_STAGE_HOST by name (pointer into the handle).
 * dawn_bundle_create_handles creates all six handles from the region and fills the six handle fields of `args` (nothing else of it);
 * DAWN_OPT_UP_BORDER is set from the defaults record when the bundle has one.  A stage missing from the file is an error that names it;
 * on any error the handles made so far are destroyed and `args` is untouched.  dawn_bundle_destroy_handles destroys the six and zeroes
 * the fields.  The region must outlive the handles.
 * DAWN_STAGE_MOTION = 7 (the motion-encode stage, dawn_motion_cfg as its "cfg") came after the format's first release and is OPTIONAL:
 * the format version stays 1, a file without the stage is as valid as before, dawn_bundle_create_handles neither needs nor reads it,
 * dawn_bundle_table / dawn_bundle_cfg take stage 7 like 0 .. 5.  A loader from before the stage refuses a file that has it, by the
 * stage number of the first such index entry. */
typedef struct dawn_bundle dawn_bundle;
enum { DAWN_STAGE_HUBERT = 0, DAWN_STAGE_POSE = 1, DAWN_STAGE_BLINK = 2, DAWN_STAGE_DECODER = 3, DAWN_STAGE_INPUTS = 4, DAWN_STAGE_UNET = 5,
       DAWN_STAGE_HOST = 6, DAWN_STAGE_MOTION = 7 };
enum { DAWN_BUNDLE_DEVICE = 0, DAWN_BUNDLE_HOST = 1 };
/* what VideoGenerator takes from the yaml and its fallbacks (UVG:277-278, 329, 340-341) */
typedef struct dawn_bundle_defaults {
    int H, fea_ch, latent_dim, max_n_frames;         /* image side, the unet's fea_ch, the PBnets' latent width, the clip-length cap */
    int sampling_step, ancestral;                    /* the default step table: "steps.ddim.<sampling_step>" (ancestral = 0) or "steps.ancestral.<..>" */
    float cond_scale; int up_border;                 /* up_border: DAWN_OPT_UP_BORDER of the unet */
    uint64_t random_seed;
    double mean[3];                                  /* mean_c as the yaml holds it (0..255); dawn_generate_args.mean3 = mean / 255 */
    float bbox6[6]; float init_pose6[6]; float init_blink2[2];
    dawn_clip_mode clip;
} dawn_bundle_defaults;
int dawn_bundle_open(const char* path, dawn_bundle** out);
void dawn_bundle_close(dawn_bundle* b);
size_t dawn_bundle_device_bytes(const dawn_bundle* b);
size_t dawn_bundle_verify_workspace_bytes(const dawn_bundle* b);
int dawn_bundle_upload(dawn_bundle* b, void* device_mem, size_t bytes, void* stream);
int dawn_bundle_verify(dawn_bundle* b, const void* device_mem, size_t bytes, void* workspace, size_t workspace_bytes, void* stream);
int dawn_bundle_table(dawn_bundle* b, int stage, const void* device_mem, const dawn_named_ptr** table, int* n);
int dawn_bundle_cfg(const dawn_bundle* b, int stage, void* out, size_t out_bytes);
int dawn_bundle_host(const dawn_bundle* b, const char* name, const void** ptr, size_t* bytes);
int dawn_bundle_create_handles(dawn_bundle* b, const void* device_mem, dawn_generate_args* args);
void dawn_bundle_destroy_handles(dawn_generate_args* args);
/* the seventh handle: the motion-encode stage from the table and the "cfg" blob (one dawn_motion_cfg) of DAWN_STAGE_MOTION.  A bundle
 * without the stage: error "stage 'motion' is missing", *m untouched.  The caller destroys it with dawn_motion_destroy, before the region goes. */
int dawn_bundle_create_motion(dawn_bundle* b, const void* device_mem, dawn_motion** m);
/* after a stream synchronise: (kind, algorithmic flops, algorithmic bytes, ms) per conv launch recorded under
 * DAWN_OPT_PROFILE; kind 0 = split 3x3, 1 = split 1x1, 2 = fp32 MFMA; returns the number of entries (and clears them) */
int dawn_ctx_profile_read(dawn_ctx* ctx, double* out4, int max_entries);
/* helpers the evaluator uses (exported for hosts that build their own orchestration) */
int dawn_chw_to_hwc(const float* in, int C, long HW, float* out, void* stream);
int dawn_rotary_tables(const float* freqs16, int n, int pos0, float* cos_out, float* sin_out, void* stream);
int dawn_rel_pos_bucket(int rel);                                     /* MT:92-109, num_buckets = max_distance = 32 (host) */
int dawn_gemm1x1_ln_inline_ok(long M, int N, int C0, int C1);       /* host: may dawn_conv_desc.ln_eps be used for this projection? */
int dawn_gemm1x1_split_ok(long M, int N, int C0, int C1);             /* host: does a 1x1 projection take the split GEMM? */

/* ---- measurement helper (bench.py; not on the product path): sustained executed TFLOP/s of an MFMA-only bf16 loop on this
 * box under its power budget.  mode 0 = zero operands, 1 = operands from registers, 2 = re-read from LDS at the 32x32x16 conv kernels'
 * ratio, 3 = v_mfma_f32_16x16x32_bf16 with the shipped 3x3 kernel's LDS ratio; operands = 16 x 256 x 8 bf16 (64 KB), scratch >= 2 * CUs * 256 floats.  Synchronises. */
int dawn_ubench_mfma_bf16(int mode, int iters, const void* operands, float* scratch, float* tflops_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
