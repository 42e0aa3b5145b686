/* C ABI of libu2seg_hip.so — the MI355X (gfx950) kernels behind the U2Seg Panoptic-FPN hot path.
 *
 * Every entry point takes raw device pointers, sizes and a hipStream_t passed as void*; nothing is
 * allocated inside (workspaces are caller-provided); the return value is 0 on success, a positive
 * hipError_t on a launch failure, a negative number on an argument the kernel cannot serve.
 * The caller is a torch.autograd.Function in u2seg_amd/layers (the reference binds its native ops
 * the same way: detectron2/layers/roi_align_rotated.py:9-46 + detectron2/layers/csrc/vision.cpp:111-116).
 *
 * Activations are NHWC bfloat16 (raw uint16 bits), statistics / losses / box arithmetic are fp32.
 * Each prototype cites the reference call site(s) it replaces (paths relative to the reference root).
 */
#ifndef U2SEG_HIP_H
#define U2SEG_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- convolution / linear family (entry points and dispatch: conv_api.hip) -------------------
 * Replaces F.conv2d in detectron2/layers/wrappers.py:127-134 (all Conv2d of backbone/resnet.py:194-210,
 * 355-358, backbone/fpn.py:141-158, meta_arch/semantic_seg.py:196-205, proposal_generator/rpn.py:127-134,
 * roi_heads/mask_head.py:242-251), nn.Linear in roi_heads/box_head.py:66-74 and roi_heads/fast_rcnn.py:236-239,
 * and (through mul/div + a flipped, transposed filter) their data gradients.
 *   out[m][n] = sum_{kh,kw,c} in[src(m,kh,kw)][c] * wt[n][kh][kw][c]   (+bias)(+=old)(relu)
 *   src: sy = oy*mul - pad_h + kh; if div > 1 the tap contributes only when sy % div == 0 and then sy /= div.
 *   stats (optional, [2][N] fp32, pre-zeroed): column sum and sum of squares of the stored bf16 outputs.
 * variant: the conv word, see below. */

/* ---- the `variant` words and the u2_conv_last_kernel codes -------------------------------------
 * Every convolution entry point takes an `int variant` that steers which kernel serves the launch.  0 = the library's own
 * choice, which is all the product path passes apart from U2_CV_STREAMK_FORBID.  A caller that passes 0 can be steered from
 * the environment instead (tests, A/B runs): the variable named with each word carries the same number.  There are three words
 * with separate encodings.  A one-bit field has one mask; a wider field has X_SHIFT and X_MASK, its value is
 * (word >> X_SHIFT) & X_MASK.  "force": wherever the kernel can serve the shape, size rules lifted; "forbid": never.
 * Where both bits of a pair are set, forbid wins unless the field says otherwise.  This block is the one place where the bits
 * are described; the values are fixed (recorded command lines carry them) and no field reaches bit 31. */

/* The conv word: u2_conv_igemm, u2_conv_dgrad_tail, U2_CONV_VARIANT.
 * Bits 0-11 choose among the conv_igemm.hip kernels, which run when no other family takes the launch. */
#define U2_CV_REG_STAGING (1u << 0)           /* register-staged operands instead of global_load_lds */
#define U2_CV_BK32 (1u << 2)                  /* K tiles of 32 channels instead of 64 */
#define U2_CV_TILE_256X128 (1u << 3)          /* 256 px x 128 ch tile, 8 waves (layers with > 64 output channels) */
#define U2_CV_RING_SHIFT 4                    /* LDS ring depth: 0 = default, 1-3 = 2-4 stages */
#define U2_CV_RING_MASK 3
#define U2_CV_WIDE_FORCE (1u << 8)            /* conv_igemm256: 256 x 256 tile, 8 waves */
#define U2_CV_WIDE_FORBID (1u << 9)
#define U2_CV_WIDE_STAGGER (1u << 10)         /* conv_igemm256 with the staggered two-group schedule */
#define U2_CV_WIDE_STAGGER_PARITY (1u << 11)  /* ... its wave groups = even / odd waves instead of waves 0-3 / 4-7 */
/* Persistent tile kernels of conv_tile.hip: 0 = automatic, 1 = 256ch x 256px ring 4, 2 = 256 x 256 ring 5, 3 = 128ch x 256px
 * ring 3, 4 = 256ch x 128px ring 3, 5 = 128ch x 256px ring 4, 6 = 64ch x 512px ring 4, 7 = 256 x 256 with whole K tiles (C % 64
 * == 0), 15 = never. */
#define U2_CV_TILE_CFG_SHIFT 12
#define U2_CV_TILE_CFG_MASK 15
#define U2_CV_TILE_CFG_NEVER 15               /* a value of the field, not a mask */
#define U2_CV_TINY_GRID (1u << 16)            /* 8 work-groups only (tests: several tiles per work-group), every persistent family */
/* Bit 17 means two things, one per kernel family: the two names below have the same value. */
#define U2_CV_STREAM_FORCE (1u << 17)         /* conv_stream.hip: force the weights-resident streaming 1x1 kernel */
#define U2_CV_HALO_TILE128 (1u << 17)         /* conv_halo.hip: 128-channel tiles also for layers with <= 64 output channels */
/* Measurement switches (ConvArgs::abl, tests/native/selftest bench2 only): the field as a whole and its bits. */
#define U2_CV_ABL_SHIFT 18
#define U2_CV_ABL_MASK 63
#define U2_CV_ABL_NO_STORES (1u << 18)        /* no output stores */
#define U2_CV_ABL_NO_STATS (1u << 19)         /* no BN statistics */
#define U2_CV_ABL_NO_EPILOGUE (1u << 20)      /* no epilogue at all */
#define U2_CV_ABL_NT_STORES (1u << 21)        /* non-temporal stores for outputs > 160 MB (measured slower, off by default) */
#define U2_CV_ABL_NO_STATS_FLUSH (1u << 22)   /* conv_halo.hip: statistics summed but their atomics not sent */
#define U2_CV_HALO_FORCE (1u << 24)           /* conv_halo.hip: halo-staged 3x3 / stride 1 / pad 1 kernel */
#define U2_CV_HALO_FORBID (1u << 25)
#define U2_CV_STREAM_FORBID (1u << 26)        /* conv_stream.hip (force: U2_CV_STREAM_FORCE) */
#define U2_CV_STREAMK_FORCE (1u << 27)        /* conv_tile.hip: stream-K form, equal shares of the (tile, half K tile) sequence */
#define U2_CV_STREAMK_FORBID (1u << 28)       /* whole tiles only; callers with several streams pass this */
#define U2_CV_HALO_SCHED_SHIFT 29             /* conv_halo.hip schedule: 0 = default; bit 0 s_setprio around the MFMA runs, */
#define U2_CV_HALO_SCHED_MASK 3               /* bit 1 sched_barrier fences (measured slower, profiles/r03_conv_halo_sched.txt) */
/* Cross-field rules.  Any bit of U2_CV_EXPLICIT_MASK (bits 0-15, the unnamed ones included) is an explicit kernel choice and
 * keeps the launch off the streaming kernel; an explicit tile configuration (U2_CV_TILE_CFG != 0) also keeps it off the halo
 * kernel. */
#define U2_CV_EXPLICIT_MASK 0xffffu

/* The wgrad word: u2_conv_wgrad, u2_conv_wgrad_into, U2_WGRAD_VARIANT.
 * Bits 0-11 belong to the per-tap kernels of conv_wgrad.hip (128 x 128 and 256 x 256 tiles). */
#define U2_WG_REG_STAGING (1u << 0)           /* register-staged operands instead of global_load_lds */
#define U2_WG_SCALAR_GATHER (1u << 1)         /* scalar LDS gathers instead of ds_read_b64_tr_b16 */
#define U2_WG_FEWER_SPLITS_SHIFT 4            /* resident work-groups (pixel splits) halved this many times */
#define U2_WG_FEWER_SPLITS_MASK 3
#define U2_WG_XCD_FORCE (1u << 6)             /* XCD-grouped launch (default: multi-tap filters over >= 200k pixels); */
#define U2_WG_XCD_FORBID (1u << 7)            /* force wins over forbid */
/* 256 x 256 tile kernel (default: 1x1 layers over >= 50k pixels with both channel counts % 256 == 0, and the 7x7 fc1); force wins
 * over forbid; U2_WG_REG_STAGING or U2_WG_SCALAR_GATHER keeps a launch off it. */
#define U2_WG_WIDE_FORCE (1u << 8)
#define U2_WG_WIDE_FORBID (1u << 11)
#define U2_WG_RING_SHIFT 9                    /* LDS ring depth of the 128 x 128 LDS-DMA form: 0 = two buffers, 1 = 3, 2 = 4 */
#define U2_WG_RING_MASK 3
#define U2_WG_HALO_FORCE (1u << 12)           /* wgrad_halo.hip: 3x3 / stride 1 / pad 1, all nine taps per work-group */
#define U2_WG_HALO_FORBID (1u << 13)
#define U2_WG_HALO_ROUNDS_SHIFT 14            /* wgrad_halo.hip: rounds of work-groups - 1 (0 = one work-group per CU) */
#define U2_WG_HALO_ROUNDS_MASK 3
#define U2_WG_ATOMICS (1u << 16)              /* fp32-atomic epilogue, never partial tiles + a reduction pass; wins over ... */
#define U2_WG_PARTIALS_FORCE (1u << 17)       /* ... the reduction pass wherever there are >= 2 pixel splits */
#define U2_WG_STREAM_FORCE (1u << 18)         /* wgrad_stream.hip: 1x1 / stride 1, the dW block in registers (default: >= 200k pixels) */
#define U2_WG_STREAM_FORBID (1u << 19)
#define U2_WG_STREAM_TINY (1u << 20)          /* wgrad_stream.hip: 8 pixel ranges only (tests) */
#define U2_WG_STREAM_CFG_SHIFT 21             /* block: 0 = automatic, 1 = 256(n) x 64(c), 2 = 64 x 256, 3 = 128 x 128, 4 = 256 x 256 */
#define U2_WG_STREAM_CFG_MASK 7
#define U2_WG_STREAM_PER_CU_SHIFT 24          /* work-groups per CU: 0 = the configuration's default */
#define U2_WG_STREAM_PER_CU_MASK 3
/* Cross-field rules.  Any of bits 0-11 (the unnamed ones included) keeps a launch off the streaming kernel, any of bits 0-10
 * off the halo kernel: the per-tap kernels' own switches ask for those kernels. */
#define U2_WG_PER_TAP_MASK_STREAM 0xfffu
#define U2_WG_PER_TAP_MASK_HALO 0x7ffu

/* The fused 1x1 backward word: u2_conv1x1_bwd_fused, u2_conv1x1_bwd_fused_bn, U2_WDGRAD_VARIANT. */
#define U2_WD_FORCE (1u << 0)                 /* lift the size rule (>= 200 000 pixels, > 128 valid output channels) */
#define U2_WD_TINY (1u << 1)                  /* 8 pixel ranges only (tests) */
#define U2_WD_NEVER (1u << 2)                 /* decline (return 1): the caller takes the separate launches */
#define U2_WD_BN_TWO_GROUPS (1u << 3)         /* _bn only: 4-wave blocks, two work-groups per CU, instead of one 8-wave group */
#define U2_WD_BN_WIDE (1u << 4)               /* _bn only: also serve N <= 512 by C <= 128 (declined otherwise: DESIGN.md 5.0) */

/* u2_conv_last_kernel: a code for the kernel family and configuration that took the launch. */
#define U2_K_TILE 100              /* conv_tile.hip, whole tiles: + tile configuration (1-7) */
#define U2_K_IGEMM256 256          /* conv_igemm256_kernel ... */
#define U2_K_IGEMM256_STAGGER 1024 /* ... + this with the staggered schedule */
#define U2_K_HALO 300              /* conv_halo.hip, 128-channel tiles */
#define U2_K_HALO_N64 301          /* conv_halo.hip, 64-channel tiles */
#define U2_K_STREAMK 500           /* conv_tile.hip, stream-K form: + tile configuration */
#define U2_K_STREAM 700            /* conv_stream.hip: + C / 32 * 10 + (1, 2, 4 waves along the pixels -> 0, 1, 2) ... */
#define U2_K_STREAM_TAIL 5         /* ... or + C / 32 * 10 + this for u2_conv_dgrad_tail */
/* conv_igemm_kernel<BK, GLDS, TM, TN, NST>: U2_K_IGEMM + BK * 10000 + TM / 64 * 1000 + TN / 64 * 100 + NST * 10 + GLDS */
#define U2_K_IGEMM 1000000
#define U2_K_WGRAD 2000            /* conv_wgrad.hip, conv_wgrad_kernel<GLDS, TR>: + GLDS * 2 + TR */
#define U2_K_WGRAD_XCD 100         /* added to U2_K_WGRAD / U2_K_WGRAD256 codes when the launch is XCD-grouped */
#define U2_K_WGRAD256 2256         /* conv_wgrad256_kernel */
#define U2_K_WGRAD_STREAM 2700     /* wgrad_stream.hip: + block configuration (1-4) */
#define U2_K_WDGRAD 2750           /* u2_conv1x1_bwd_fused: + 1 (N <= 256 by C <= 64) / + 2 (N <= 512 by C <= 128) */
#define U2_K_WDGRAD_BN 2760        /* u2_conv1x1_bwd_fused_bn: + 1 default, + 2 U2_WD_BN_TWO_GROUPS, + 3 U2_WD_BN_WIDE block */
#define U2_K_WGRAD_HALO 2900       /* wgrad_halo.hip */

int u2_conv_igemm(const void* in, const void* wt, void* out, const float* bias, float* stats,
                  int B, int Hin, int Win, int C, int in_ld, int Hout, int Wout, int N, int out_ld,
                  int KH, int KW, int pad_h, int pad_w, int mul, int div, int relu, int accumulate,
                  int variant, void* stream);

/* Weight gradient: dw[n][kh][kw][c] += sum_m dy[m][n] * x[src(m,kh,kw)][c]; fp32 atomics, dw pre-zeroed.
 * variant: the wgrad word, see above. */
int u2_conv_wgrad(const void* x, const void* dy, float* dw, int B, int Hin, int Win, int C, int x_ld,
                  int Hout, int Wout, int N, int dy_ld, int KH, int KW, int pad_h, int pad_w,
                  int stride, int variant, void* stream);
/* Same reduction accumulated into a caller-laid-out destination: dw[n * dw_stride_n + tap * dw_stride_tap + c * dw_stride_c]
 * for n < n_valid, c < c_valid (tap = kh * KW + kw).  With (Cin*KH*KW, 1, KH*KW) the destination is the reference's
 * own [N][Cin][KH][KW] parameter gradient (torch.nn.Conv2d.weight.grad, layers/wrappers.py:127-134), so the gradient
 * lands in the optimizer's flat arena without a temporary, a permute or an accumulate pass. */
int u2_conv_wgrad_into(const void* x, const void* dy, float* dw, int B, int Hin, int Win, int C, int x_ld,
                       int Hout, int Wout, int N, int dy_ld, int KH, int KW, int pad_h, int pad_w,
                       int stride, int n_valid, int c_valid, long long dw_stride_n, int dw_stride_tap,
                       int dw_stride_c, int variant, void* stream);

/* Both gradients of a 1x1 / stride-1 convolution in ONE pass over dy (autograd's conv backward behind layers/wrappers.py:127-134
 * for the expanding 1x1 layers of the bottlenecks, backbone/resnet.py:194-203): dx[m][c] = sum_n dy[m][n] wt[c][n] (bf16, all dx_ld
 * physical channels written) and dw[n * dw_stride_n + c * dw_stride_c] += sum_m dy[m][n] x[m][c] (fp32, n < n_valid, c < c_valid).
 * wt is the data-gradient layout of the filter, [C][wt_ld] with n contiguous (u2_weight_layout mode 1).  Returns 0 when launched,
 * 1 when the shape is not served (blocks of N <= 256 by C <= 64 or N <= 512 by C <= 128 over >= 200 000 pixels) - the caller then
 * issues u2_conv_igemm + u2_conv_wgrad_into.  variant: the fused 1x1 backward word, see above. */
int u2_conv1x1_bwd_fused(const void* x, const void* dy, const void* wt, void* dx, float* dw, int M, int C, int x_ld, int N, int dy_ld,
                         int wt_ld, int dx_ld, int n_valid, int c_valid, long long dw_stride_n, int dw_stride_c, int variant,
                         void* stream);

/* The same pass for a layer whose output y feeds a batch normalisation (layers/batch_norm.py:169-197 behind layers/wrappers.py:
 * 127-134: conv3 + norm of a bottleneck, the projection shortcut): the normalisation's backward apply step
 * dy[m][n] = k1[n] dz[m][n] + k2[n] y[m][n] + k3[n] (u2_norm_bwd_apply with relu = 0, coefficients of u2_bn_finalize_bwd) is
 * evaluated on the staged rows instead of being written and read back; dx and dw are those of u2_conv1x1_bwd_fused on that dy.
 * Served: N <= 256 by C <= 64 (same size rule); returns 1 otherwise - the caller then runs u2_norm_bwd_apply followed by
 * u2_conv1x1_bwd_fused (or the two separate launches).  variant: the fused 1x1 backward word, see above. */
int u2_conv1x1_bwd_fused_bn(const void* x, const void* dz, const void* y, const float* k1, const float* k2, const float* k3,
                            const void* wt, void* dx, float* dw, int M, int C, int x_ld, int N, int dy_ld, int wt_ld, int dx_ld,
                            int n_valid, int c_valid, long long dw_stride_n, int dw_stride_c, int variant, void* stream);

/* The data gradient of a bottleneck's conv1 (1x1, stride 1: u2_conv_igemm with KH = KW = 1, mul = div = 1, no bias) whose input
 * is the previous block's output (backbone/resnet.py:194-210), with that block's tail reduce in its epilogue: with g1 the value
 * u2_conv_igemm would have stored, dz = relu_bits * bf16(g1 + dout2) and sums[0][n] += sum dz, sums[1][n] += sum dz (y - mean) invstd
 * - u2_conv_igemm followed by u2_norm_bwd_reduce(dout = g1, dout2, dz_out, mask_is_bits = 1) in one launch, dz bit for bit and
 * the sums up to the order of the fp32 additions; g1 is never stored.  in: [B][H][W][in_ld] (C reduction channels), wt: [N][C]
 * data-gradient layout, dout2 / y / dz: [B * H * W][N] (out_ld == N), bits: [B * H * W][N / 8] as u2_affine_act writes them,
 * sums: [2][N] fp32 zeroed by the caller.  Served: (C, N) = (64, 256), (128, 512), (256, 1024) on maps the streaming kernel
 * takes.  Returns 0 when launched, 1 when not served - nothing is written, the caller issues the two launches.
 * variant: the conv word, see above (U2_CV_TINY_GRID, U2_CV_STREAM_FORCE, U2_CV_STREAM_FORBID and U2_CV_EXPLICIT_MASK apply). */
int u2_conv_dgrad_tail(const void* in, const void* wt, const void* dout2, const void* y, const void* bits, const float* mean,
                       const float* invstd, void* dz, float* sums, int B, int H, int W, int C, int in_ld, int N, int out_ld,
                       int variant, void* stream);

/* Test / debugging aid: a code for the kernel (family, tile configuration) the most recent u2_conv_igemm or u2_conv_wgrad
 * call on this thread selected (the U2_K_ codes above).  With variant 0 the selection can be steered through the
 * environment variables U2_CONV_VARIANT / U2_WGRAD_VARIANT / U2_WDGRAD_VARIANT (the variant words above). */
int u2_conv_last_kernel(void);

/* The only device memory the library owns (conv_scratch.hip): the conv kernels' scratch (stream-K hand-over slots of u2_conv_igemm, partial tiles of
 * u2_conv_wgrad), one block per (device, stream), allocated on first need at the size of that launch and grown on demand.  This
 * call drains the streams concerned and frees every block (the next launch that needs one allocates again); returns the number
 * of blocks freed.  The reference's ops (ATen conv behind layers/wrappers.py:127-134) take such workspaces from torch's caching
 * allocator, where torch.cuda.empty_cache() releases them - this is the equivalent for a plain C ABI. */
int u2_release_scratch(void);

/* ---- grouped 3x3 convolution (conv_grouped.hip) -------------------------------------------------
 * F.conv2d(groups = G) behind layers/wrappers.py:127-134 for conv2 of a ResNeXt bottleneck (backbone/resnet.py:155-166), its
 * data gradient and its weight gradient.  Activations NHWC bf16 with C == N physical channels, C % 32 == 0, cg = C / groups;
 * filter 3x3, pad 1, stride 1 or 2, Hout = (H + 2 - 3) / stride + 1.  All three read the fp32 parameter in the reference's own
 * layout w[N][cg][3][3]; no bf16 layout exists outside the launch:
 *   W'[n][c][t] = bf16(w[n][c][t] * (scale ? scale[n] : 1.0f))                 one fp32 multiply, one rounding (the FrozenBN fold)
 *   fwd:   out[b,ho,wo,n] = bf16(relu?(sum_{t, c in group(n)} in[...][c] W'[n][c - c0][t] + bias[n])), fp32 sum and bias add;
 *          stats ([2][N] fp32, zeroed by the caller): column sum and sum of squares of the STORED values, fp32 atomics
 *   dgrad: dx[b,h,w,c] = bf16(sum_{t, n in group(c)} dz[b,(h+1-kh)/s,(w+1-kw)/s,n] W'[n][c - c0][t]) over the taps whose source
 *          coordinate is integral and inside the map; every element of dx is written.  H, W: the INPUT map (dx)
 *   wgrad: dw[n][c][kh][kw] += (scale ? scale[n] : 1) * sum_{b,ho,wo} dz[b,ho,wo,n] x[b,ho*s+kh-1,wo*s+kw-1,c0+c], fp32 atomics
 *          into the caller's [N][cg][3][3] buffer (the arena slot or a zeroed tensor)
 * Served: groups >= 2, C = groups * cg, cg in {4, 8, 16, 32, 64}.  Returns 0 when launched, 1 when the shape is not served
 * (nothing is written). */
int u2_gconv3x3_fwd(const void* in, const float* w, const float* scale, const float* bias, void* out, float* stats, int B, int H,
                    int W, int C, int groups, int stride, int relu, void* stream);
int u2_gconv3x3_dgrad(const void* dz, const float* w, const float* scale, void* dx, int B, int H, int W, int C, int groups,
                      int stride, void* stream);
int u2_gconv3x3_wgrad(const void* x, const void* dz, const float* scale, float* dw, int B, int H, int W, int C, int groups,
                      int stride, void* stream);

/* fp32 master weights [N][Cin][T] -> bf16 kernel layouts: mode 0 [N][T][Cp] (forward / wgrad), mode 1 [Cp][T][Npad] with the
 * taps reversed (data gradient), mode 2 [T][Cp][Npad] (data gradient of a fully connected conv). Zero padded. */
int u2_weight_layout(const float* w, void* out, int N, int Cin, int T, int Cp, int Npad, int mode, void* stream);
/* The same for a whole table of (parameter, layout) pairs in one launch - run once after the optimizer step on the flat
 * parameter arena (base + src_offset floats), so that no per-layer layout launch is left in the forward/backward pass. */
typedef struct U2LayoutDesc {
  long long src_offset; /* floats from `base` to the [N][Cin][T] fp32 parameter */
  void* dst;            /* device pointer of the bf16 layout */
  int N, Cin, T, Cp, Npad, mode;
  int block_begin;      /* first work-group of this entry: prefix sum of blocks(entry) = mode 0: N * ceil(Cp/64);
                           modes 1, 2 (need Cp == Cin): ceil(Npad/64) * ceil(Cin*T/64); mode 3 (this table only): dst is an
                           fp32 vector of N elements = the source rounded through bf16 (a conv bias under autocast),
                           ceil(N/4096) blocks; mode 0 with T == 1 and Cp == Cin: ceil(N*Cp/4096) */
  int reserved;
} U2LayoutDesc;
int u2_weight_layout_batched(const float* base, const U2LayoutDesc* table, int n_entries, int total_blocks, void* stream);

/* ---- normalisation / activation (norm.hip) ----------------------------------------------------
 * Replaces nn.SyncBatchNorm / nn.GroupNorm / relu_ chosen by detectron2/layers/batch_norm.py:169-197. */
int u2_colstats(const void* x, float* out /*[slots][2][C]*/, int slots, int rows_per_slot, int C, int ld, void* stream);
/* u2_colstats with the additions in a fixed order (no atomics): the same call on the same input gives the same bits from run to
 * run, which u2_colstats does not.  part: scratch float32 [slots][nchunk][2][C], written in full; out [slots][2][C] is written,
 * not added to.  Pass 1 sums rows_per_slot / nchunk (rounded up) rows per work-group, pass 2 the chunks in order.  C % 8 == 0,
 * 8 <= C <= 2048, ld % 8 == 0, x 16-byte aligned, 1 <= nchunk <= 65535; -1 otherwise (nothing launched). */
int u2_colstats_ordered(const void* x, float* part, float* out, int slots, int rows_per_slot, int C, int ld, int nchunk,
                        void* stream);
/* dst[c] += sum over rows of x[row][c] for c < n_valid (x: [rows][ld] bf16, C physical channels): the bias gradient of a conv /
 * linear layer (autograd's sum over the output gradient behind layers/wrappers.py:127-134) accumulated straight into the
 * parameter's fp32 gradient storage - no temporary, no AccumulateGrad add. */
int u2_colsum_add(const void* x, float* dst, int rows, int C, int ld, int n_valid, void* stream);
/* nn.GroupNorm finalize (layers/batch_norm.py:189 "GN", semantic_seg.py:196-205). fwd: stats [B][2][C] (u2_colstats per image)
 * -> mean / invstd / scale / shift [B][C], n = H*W*(C/groups) elements per group. bwd: sums [B][2][C] (u2_norm_bwd_reduce)
 * -> k1/k2/k3 [B][C] for u2_norm_bwd_apply and dgamma / dbeta [C] summed over the images in order; accumulate != 0: added to
 * what dgamma / dbeta hold (the optimizer's gradient slices: no temporary, no AccumulateGrad add). */
int u2_gn_finalize_fwd(const float* stats, const float* gamma, const float* beta, float n, float eps, int B, int C, int groups,
                       float* mean, float* invstd, float* scale, float* shift, void* stream);
int u2_gn_finalize_bwd(const float* sums, const float* gamma, const float* mean, const float* invstd, float n, int B, int C,
                       int groups, float* k1, float* k2, float* k3, float* dgamma, float* dbeta, int accumulate, void* stream);
/* count: elements per channel behind `sums`; count_dev (optional, device, 1 float) overrides it - SyncBN all-reduces the
 * per-rank counts together with the sums, because ranks pad their batches to different sizes (nn.SyncBatchNorm does). */
int u2_bn_finalize_fwd(const float* sums, float count, const float* count_dev, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float momentum, float eps, float* mean, float* invstd, float* scale,
                       float* shift, int C, void* stream);
/* relu_bits (optional, uint8 [slots * rows_per_slot][C / 8], needs ld == C and C / 8 dividing 256): bit e of byte c is
 * out[row][8 c + e] > 0 - what the backward pass of a residual block's tail needs of the activation, in 1/16 of its bytes. */
int u2_affine_act(const void* x, const float* scale, const float* shift, const void* resid, void* out, int slots,
                  int rows_per_slot, int C, int ld, int relu, void* relu_bits, void* stream);
/* backbone/fpn.py:141-158 in one pass: out = bf16(x * scale + shift) + nearest_x2(top), top [B][H/2][W/2][C]: the lateral conv's
 * BatchNorm apply fused with the top-down upsample-add (bit-identical to u2_affine_act followed by u2_fpn_upsample_add_fwd). */
int u2_affine_upadd(const void* x, const float* scale, const float* shift, const void* top, void* out, int B, int H, int W,
                    int C, int relu, void* stream);
int u2_norm_bwd_reduce(const void* dout, const void* mask, const void* x, const float* mean, const float* invstd,
                       float* out /*[slots][2][C]*/, int slots, int rows_per_slot, int C, int ld, int relu,
                       const float* mask_scale, const float* mask_shift, const void* dout2, void* dz_out, const void* dout3,
                       int mask_is_bits, void* stream);
/* mask_scale/mask_shift [slots][C] (optional, both or neither): recompute the ReLU mask as x*scale+shift > 0 - the
 * expression u2_affine_act evaluated in the forward pass - instead of reading the activation `mask` (which may be NULL).
 * u2_norm_bwd_reduce only: dz_out (optional) receives the masked gradient dz = (dout [+ dout2]) * mask, so that
 * u2_norm_bwd_apply can run on (dz, x) with relu = 0 and dz doubles as the residual branch's gradient; dout2 (optional,
 * needs dz_out) is a second incoming gradient summed on the fly (resnet.py:204-210: the block output feeds the next
 * block's conv1 and its identity shortcut); dout3 (optional, needs dout2) a third one (the last block of a stage also feeds
 * the FPN lateral conv, backbone/fpn.py:141-146); mask_is_bits: `mask` is the relu_bits array of u2_affine_act (needs dz_out). */
int u2_bn_finalize_bwd(const float* sums, float count, const float* count_dev, const float* gamma, const float* mean, const float* invstd,
                       const float* local_sums, float* dgamma, float* dbeta, float* k1, float* k2, float* k3, int C,
                       int accumulate /* dgamma/dbeta += instead of = (parameter gradient arena) */, void* stream);
int u2_norm_bwd_apply(const void* dout, const void* mask, const void* x, const float* k1, const float* k2,
                      const float* k3, void* dx, void* dres, int slots, int rows_per_slot, int C, int ld, int relu,
                      const float* mask_scale, const float* mask_shift, void* stream);
/* Round 4: nn.SyncBatchNorm's finalize and apply steps (layers/batch_norm.py:169-197 + the residual add / relu_ of
 * backbone/resnet.py:204-210) as ONE launch each way - u2_bn_finalize_fwd + u2_affine_act (slots = 1), resp. u2_bn_finalize_bwd +
 * u2_norm_bwd_apply, with identical results: every thread derives the coefficients of its channels from the column sums, one
 * work-group writes mean / invstd / scale / shift and the running statistics (forward) or adds dgamma / dbeta (backward).
 * k123: [3][C] scratch, only written when C is not served by the one-launch form (C / 8 must divide 256). */
int u2_bn_act_fused(const void* x, const float* sums, float count, const float* count_dev, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, float* mean, float* invstd, float* scale,
                    float* shift, const void* resid, void* out, int rows, int C, int ld, int relu, void* relu_bits, void* stream);
int u2_bn_bwd_apply_fused(const float* sums, float count, const float* count_dev, const float* gamma, const float* mean,
                          const float* invstd, const float* local_sums, float* dgamma, float* dbeta, float* k123, int accumulate,
                          const void* dout, const void* mask, const void* x, void* dx, void* dres, int rows, int C, int ld,
                          int relu, const float* mask_scale, const float* mask_shift, void* stream);
/* Precise BatchNorm statistics (fvcore.nn.precise_bn.update_bn_stats behind detectron2/engine/hooks.py:567-636): the population
 * mean and variance of every training-mode BN layer over K batches, from the batch statistics a momentum-1.0 training forward
 * leaves in running_mean / running_var.  One row per layer; the table is built once per pass.  The layer's batch size b
 * (N * H * W of its input) is derived on the device from the padded canvas: b = n * ceil(h / stride) * ceil(w / stride). */
typedef struct {
  float* running_mean;  /* [channels] fp32: this iteration's batch mean (update); the population mean (finalize writes) */
  float* running_var;   /* [channels] fp32: the batch's unbiased variance (update); the population variance (finalize writes) */
  int offset;           /* first channel of the layer in the packed accumulators */
  int channels;
  int stride;           /* spatial stride of the layer's map relative to the padded canvas */
  int reserved;
} U2PreciseBnLayer;
/* acc: fp64 [2][total_channels] (A = sum b * mean, Q = sum b * mean^2 + (b - 1) * var), tot: fp64 [n_layers] (T = sum b), zeroed
 * by the caller before the first update.  One work-group per layer, one thread per channel: no atomics, bit-reproducible.
 * (n, h, w): images and padded canvas of this iteration's batch. */
int u2_bn_precise_update(const U2PreciseBnLayer* table, int n_layers, double* acc, double* tot, int total_channels, int n, int h,
                         int w, void* stream);
/* running_mean = A / T, running_var = Q / T - (A / T)^2 (population variance, no Bessel factor), rounded once to fp32. */
int u2_bn_precise_finalize(const U2PreciseBnLayer* table, int n_layers, const double* acc, const double* tot, int total_channels,
                           void* stream);
int u2_relu_bwd(const void* dout, const void* out, void* dz, long long numel, void* stream);
/* The same with the bias gradient of the layer in the same pass: dst[c] += sum over rows of dz[row][c] for c < n_valid (dz: [rows][ld],
 * C physical channels; zeros: C floats of 0).  Replaces u2_relu_bwd + u2_colsum_add for a conv with bias and ReLU. */
int u2_relu_bwd_colsum(const void* dout, const void* out, void* dz, float* dst, const float* zeros, int rows, int C, int ld, int n_valid,
                       void* stream);
/* out = a + b (+ c (+ d)) on bf16 tensors of numel elements (numel % 8 == 0), summed in fp32 and rounded once; out may alias an
 * input. The gradient sum autograd would otherwise make with k - 1 separate adds where a tensor has k consumers (the FPN
 * outputs feed the RPN head, the ROI poolers and the semantic head: meta_arch/panoptic_fpn.py:105-131). */
int u2_add_n(const void* a, const void* b, const void* c, const void* d, void* out, long long numel, void* stream);

/* The kernel-layout weight gradient of a multi-tap convolution, scratch fp32 [Npad][T][Cp] (u2_conv_wgrad), accumulated into the
 * parameter's own gradient storage fp32 [N][Cin][T] (= [Cout, Cin, kh, kw], the optimizer arena): grad[n][c][t] += scratch[n][t][c]
 * for n < N, c < Cin.  Replaces the strided `grad.add_(scratch.view(...).permute(0, 3, 1, 2))` of autograd's AccumulateGrad
 * (engine/train_loop.py:479-521 leaves that accumulation to torch). */
int u2_wgrad_permute_add(const float* scratch, float* grad, int N, int Cin, int T, int Cp, void* stream);

/* ---- training through FrozenBatchNorm2d (frozen.hip) --------------------------------------------
 * layers/batch_norm.py:13-100: y * scale + shift with fixed scale = weight * rsqrt(running_var + eps).  The scale is folded into
 * the weights of the convolution in front of the norm, W'[n][c][t] = bf16(w[n][c][t] * s[n]) (one fp32 product, one rounding to
 * bf16), the shift rides as the conv epilogue's fp32 bias.  One launch writes both kernel layouts of W' for a whole table of
 * layers: fwd = [N][T][Cp] (u2_weight_layout mode 0), dgrad = [Cp][T][Npad] with the taps reversed (mode 1); either may be NULL.
 * Output channels N..Npad-1 of dgrad are written as zeros; input channels Cin..Cp-1 of both are NOT written (the caller
 * allocates the layouts zeroed once).  Cp and Npad must be even (bf16 pairs are stored; an odd entry is skipped).  An entry owns ceil(Npad / 64) * ceil(Cin * T / 64) work-groups from block_begin on. */
typedef struct U2FrozenFoldDesc {
  const float* w;   /* [N][Cin][T] fp32 master weights */
  const float* s;   /* [N] fp32 scale */
  void* fwd;        /* bf16 [N][T][Cp] or NULL */
  void* dgrad;      /* bf16 [Cp][T][Npad] or NULL */
  int N, Cin, T, Cp, Npad;
  int block_begin;  /* prefix sum of the entries' work-group counts */
  int reserved[2];
} U2FrozenFoldDesc;
int u2_frozen_fold(const U2FrozenFoldDesc* table, int n_entries, int total_blocks, void* stream);
/* The transpose of the fold: grad[n][c][t] += s[n] * scratch[n][t][c] for n < N, c < Cin - the kernel-layout weight gradient of W'
 * (u2_conv_wgrad, fp32 [Npad][T][Cp]) scaled (one fp32 rounding) and accumulated (one more) into the parameter's own gradient
 * storage fp32 [N][Cin][T].  -2: T * (Cp + 1) floats exceed 64 KB of LDS (nothing launched). */
int u2_frozen_wgrad_scale_add(const float* scratch, const float* s, float* grad, int N, int Cin, int T, int Cp, void* stream);

/* ---- pooling / resampling (pool_resize.hip) ----------------------------------------------------
 * backbone/resnet.py:358 (max_pool2d 3x3 s2 p1), backbone/fpn.py:153-155 (nearest x2 + add),
 * meta_arch/semantic_seg.py:206-211 (bilinear x2), meta_arch/rcnn.py:223-234 (normalise + pad) feeding the stem. */
int u2_maxpool3x3s2_fwd(const void* x, void* y, void* idx, int B, int H, int W, int C, void* stream);
int u2_maxpool3x3s2_bwd(const void* dy, const void* idx, void* dx, int B, int H, int W, int C, void* stream);
/* Round 6: the stem's tail - norm -> relu_ -> max_pool2d (backbone/resnet.py:355-359, layers/batch_norm.py:169-197) - without the
 * 550 MB activation between the normalisation and the pool.  Forward: y / idx of u2_maxpool3x3s2_fwd applied to
 * u2_affine_act(x, scale, shift, relu = 1), bit for bit (the nine taps are normalised, rounded to bf16 and compared as the two
 * launches do).  Backward: u2_norm_bwd_reduce / u2_norm_bwd_apply (mask recomputed from x * mask_scale + mask_shift > 0) on the
 * gradient u2_maxpool3x3s2_bwd would have stored, which is rebuilt per input pixel from dy / idx instead:
 * sums[0][c] += sum dz, sums[1][c] += sum dz * (x - mean) * invstd (fp32 [2][C], zeroed by the caller); dx = k1 dz + k2 x + k3 with
 * the coefficients of u2_bn_finalize_bwd.  x: [B][H][W][C] bf16 conv output, y / idx / dy: [B][Ho][Wo][C]; C / 8 must divide 256. */
int u2_affine_relu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, void* idx, int B, int H, int W,
                               int C, void* stream);
int u2_affine_relu_maxpool_bwd_reduce(const void* dy, const void* idx, const void* x, const float* mean, const float* invstd,
                                      const float* mask_scale, const float* mask_shift, float* sums, int B, int H, int W, int C,
                                      void* stream);
int u2_affine_relu_maxpool_bwd_apply(const void* dy, const void* idx, const void* x, const float* k1, const float* k2,
                                     const float* k3, const float* mask_scale, const float* mask_shift, void* dx, int B, int H, int W,
                                     int C, void* stream);
int u2_fpn_upsample_add_fwd(const void* lateral, const void* top, void* out, int B, int H, int W, int C, void* stream);
int u2_fpn_upsample_add_bwd(const void* dout, void* dtop, int B, int H, int W, int C, void* stream);
int u2_bilinear_up2_fwd(const void* x, const void* addend /*nullable, out = up2(x) + addend*/, void* out, int B, int H,
                        int W, int C, void* stream);
int u2_bilinear_up2_bwd(const void* dout, void* dx, int B, int H, int W, int C, void* stream);
int u2_stem_im2col(const void* img, int is_uint8, const float* mean, const float* stdv, void* col, int b, int h, int w,
                   int Hpad, int Wpad, int KP, void* stream);
/* Gradient of p6 = p5[:, ::2, ::2, :] (LastLevelMaxPool, detectron2/modeling/backbone/fpn.py:188-200): g bf16 [B][ceil(H/2)][ceil(W/2)][C]
 * -> dx bf16 [B][H][W][C] = g at even (y, x), zero elsewhere.  C % 8 == 0. */
int u2_subsample2_bwd(const void* g, void* dx, int B, int H, int W, int C, void* stream);
/* ImageList.from_tensors(gt_sem_seg, size_divisibility, ignore_value) (detectron2/structures/image_list.py:70-122 as called by
 * modeling/meta_arch/panoptic_fpn.py:118-126) for the label maps of a batch in one launch: out uint8 [n_imgs][Hpad][Wpad]
 * (16-byte aligned, Wpad % 16 == 0) = the image's labels (int64 if is_int64, else uint8; host arrays of device pointers / sizes,
 * h <= Hpad, w <= Wpad) in the top-left corner, `pad` elsewhere. */
int u2_label_pad_batch(const void* const* imgs, const int* hs, const int* ws, int n_imgs, int is_int64, void* out, int Hpad,
                       int Wpad, int pad, void* stream);
/* All images of the batch (host arrays of device pointers / sizes; images may differ in size) in one launch. */
int u2_stem_im2col_batch(const void* const* imgs, const int* hs, const int* ws, int n_imgs, int is_uint8, const float* mean,
                         const float* stdv, void* col, int Hpad, int Wpad, int KP, void* stream);
/* The same convolution without the matrix (stem_conv.hip): out bf16 [n_imgs][Ho][Wo][64] = conv of the normalised, zero-padded
 * images with wk bf16 [64][KP = 160] (K order (kh, kw, c), columns 147..159 zero); stats (nullable) fp32 [2][64] accumulates the
 * column sums and sums of squares of the stored output.  Operand values are those of u2_stem_im2col_batch bit for bit; the fp32
 * summation order differs from the GEMM's.  Returns 1 and launches nothing for a call it does not serve (N != 64, KP != 160, an
 * output of 4 GB or more): the caller takes the im2col path. */
int u2_stem_conv_fwd(const void* const* imgs, const int* hs, const int* ws, int n_imgs, int is_uint8, const float* mean,
                     const float* stdv, const void* wk, void* out, float* stats, int Hpad, int Wpad, int N, int KP, void* stream);
/* Its weight gradient: dw fp32 [64][KP] += sum over pixels of dy[m][n] * a[m][k], dy bf16 [n_imgs][Ho][Wo][64]; columns 147..159
 * are left alone.  One flush of fp32 atomics per persistent work-group.  Same answer 1 for a call it does not serve. */
int u2_stem_conv_wgrad(const void* const* imgs, const int* hs, const int* ws, int n_imgs, int is_uint8, const float* mean,
                       const float* stdv, const void* dy, float* dw, int Hpad, int Wpad, int N, int KP, void* stream);

/* ---- losses (losses.hip) -----------------------------------------------------------------------
 * meta_arch/semantic_seg.py:255-267, roi_heads/fast_rcnn.py:307-347,424-463, roi_heads/mask_head.py:33-112,
 * proposal_generator/rpn.py:366-429, modeling/box_regression.py:43-76. */
/* grad_acc [B][h][w][LP] fp32 is overwritten with the un-normalised logit gradient (no pre-zeroing needed);
 * loss_sum / valid_cnt are accumulated (pre-zeroed by the caller). */
int u2_semseg_upsample_ce(const void* logits, const void* target, float* grad_acc, float* loss_sum, float* valid_cnt,
                          int B, int h, int w, int LP, int NC, int ignore, void* stream);
int u2_scale_to_bf16(const float* acc, const float* num, const float* den, float mult, void* out, long long n,
                     void* stream);
int u2_softmax_ce(const void* logits, const void* labels, void* dlogits, float* loss_sum, int R, int NC, int LP,
                  float gscale, void* stream);
/* u2_softmax_ce plus the classification counts of fast_rcnn.py:88-115, made by the same kernel body (dlogits bit-identical):
 * counters[0..4] += rows, pred == gt, fg (0 <= gt < bg_label), fg and pred == gt, fg and pred == bg_label, with pred = argmax
 * over the NC valid columns (lowest index among equal maxima).  int32, integer atomics, one per counter and work-group (per
 * wave where LP > 1024 or LP % 8 != 0); R == 0 adds nothing.  NaN logits are outside the contract. */
int u2_softmax_ce_stats(const void* logits, const void* labels, void* dlogits, float* loss_sum, int R, int NC, int LP,
                        float gscale, int* counters, int bg_label, void* stream);
/* (u2_mask_predict_bce: phased_side = 0: x / dx are [N][P][C] in pixel order; phased_side = S2 (P = S2 * S2): they are the
 * 2x2 / stride-2 deconvolution's unshuffled GEMM output [N][S2/2][S2/2][2][2][C], target / logit_out stay in pixel order.
 * dx, dWp, dbp, loss_sum may each be NULL (not produced): the forward pass asks for the loss alone, the backward pass for the
 * gradients with gmul = the loss's upstream gradient, a device scalar the gradient scale gscale is multiplied with.) */
int u2_mask_predict_bce(const void* x, const float* Wp, const float* bp, const void* cls, const void* target, void* dx,
                        float* dWp, float* dbp, float* loss_sum, void* logit_out, int N, int P, int C, float gscale,
                        int phased_side, const float* gmul, void* stream);
/* The loss-only form of u2_mask_predict_bce plus the counts of mask_head.py:90-102 over the rounded logit z and the target t:
 * counters[0..3] += (z > 0 and t == 0), (z <= 0 and t != 0), (t != 0), positions.  One integer atomic per counter and
 * work-group. */
int u2_mask_predict_bce_stats(const void* x, const float* Wp, const float* bp, const void* cls, const void* target,
                              float* loss_sum, int* counters, int N, int P, int C, int phased_side, void* stream);
/* counters[0] += #(labels == 1), counters[1] += #(labels == 0) over n int8 labels (rpn.py:396-403 on the subsampled labels). */
int u2_count_labels_i8(const void* labels, long long n, int* counters, void* stream);
/* proposal_generator/rpn.py:366-429, one feature level.  dlt == NULL (and ddlt == NULL, A == 3): `obj` is the output of the
 * objectness and anchor-delta 1x1 convs run as ONE conv (columns 0-2 objectness, 3-14 deltas of an LPo-wide NHWC map) and dobj
 * receives both gradients in the same columns - the map their common input's gradient is then formed from by one data-gradient
 * conv instead of two and a sum. */
int u2_rpn_loss_level(const void* obj, const void* dlt, const void* labels, const int* match, const float* gt,
                      const float* anchors, void* dobj, void* ddlt, float* loss, int B, int HW, int A, int LPo, int LPd,
                      int Atot, int lvl_off, int G, float gscale, void* stream);
/* u2_rpn_loss_level with the localisation loss options (MODEL.RPN.BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA, BBOX_REG_WEIGHTS): same
 * arguments, layouts (separate maps, or dlt == ddlt == NULL for the fused A == 3 map) and objectness part.  The positives' deltas
 * are scored by `kind` (the U2_BOXLOSS_* codes below) with the anchor as the source box: SMOOTH_L1 on
 * delta - get_deltas(anchor, gt; weights), quadratic below beta and plain L1 at beta == 0; GIOU / DIOU / CIOU on
 * apply_deltas(delta, anchor; weights, scale_clamp) against the matched gt, the gradient taken through the decode (0 through a
 * clamped dw / dh, CIoU's alpha constant).  The delta gradient is exactly 0 for anchors whose label is not 1 and in every pad
 * column; the launch writes the whole gradient map(s).  With kind SMOOTH_L1, beta 0 and unit weights it returns
 * u2_rpn_loss_level's bits.  An unknown kind, beta < 0 or a weight <= 0 returns -1. */
int u2_rpn_loss_level_opt(int kind, const void* obj, const void* dlt, const void* labels, const int* match, const float* gt,
                          const float* anchors, void* dobj, void* ddlt, float* loss, int B, int HW, int A, int LPo, int LPd,
                          int Atot, int lvl_off, int G, float gscale, float wx, float wy, float ww, float wh, float beta,
                          float scale_clamp, void* stream);
int u2_box_reg_l1(const void* pred, const float* prop, const float* gtb, const void* labels, void* dpred, float* loss,
                  int R, int LP, int bg_label, float wx, float wy, float ww, float wh, float gscale, void* stream);
/* FastRCNNOutputLayers.sigmoid_cross_entropy_loss (roi_heads/fast_rcnn.py:386-422) in the layout of u2_softmax_ce: logits bf16
 * [R][LP], NC = K + 1 valid columns of which the last is the background (it takes no part), labels int64.  Per foreground
 * column c < NC - 1, with t = (labels[r] == c) and w = class_weight[c] (fp32 [>= NC - 1]; NULL = 1, the federated mask otherwise):
 * loss_sum += w (max(x, 0) - x t + log1p(exp(-|x|))),  dlogits = (sigmoid(x) - t) w gscale; dlogits is exactly 0 in the
 * background column, in the pad columns (whatever they hold) and where w == 0.  counters (NULL = none): the five counts of
 * u2_softmax_ce_stats, same definition (argmax over all NC valid logits).  One float atomic per work-group; R == 0 launches
 * nothing. */
int u2_sigmoid_ce(const void* logits, const void* labels, const float* class_weight, void* dlogits, float* loss_sum, int R,
                  int NC, int LP, float gscale, int* counters, int bg_label, void* stream);
/* The box heads' other regression losses (modeling/box_regression.py:310-369) over foreground rows (0 <= label < bg_label),
 * class agnostic: pred bf16 [R][LP] with 4 valid columns.  kind U2_BOXLOSS_SMOOTH_L1: smooth-L1 with beta > 0 on
 * pred - get_deltas(prop, gtb).  GIOU / DIOU / CIOU: the loss of layers/losses.py (GIoU: 1 - I/(U + eps) + (C - U)/(C + eps),
 * eps = 1e-7 throughout) on apply_deltas(pred, prop) (box_regression.py:78-116: deltas / weights, dw and dh clamped at
 * scale_clamp from above) against gtb; dpred is the gradient through the decode (0 through a clamped dw / dh; CIoU's alpha
 * constant), times gscale, and 0 in background rows and in columns >= 4.  loss is accumulated.  An unknown kind, or smooth-L1
 * with beta <= 0 (u2_box_reg_l1 serves that), returns -1. */
#define U2_BOXLOSS_SMOOTH_L1 0
#define U2_BOXLOSS_GIOU 1
#define U2_BOXLOSS_DIOU 2
#define U2_BOXLOSS_CIOU 3
int u2_box_reg_loss(int kind, const void* pred, const float* prop, const float* gtb, const void* labels, void* dpred,
                    float* loss, int R, int LP, int bg_label, float wx, float wy, float ww, float wh, float beta,
                    float scale_clamp, float gscale, void* stream);

/* u2_box_reg_loss for class-specific regression (cls_agnostic_bbox_reg = False): pred bf16 [R][LP] with 4 * bg_label valid
 * columns; a foreground row of label c reads columns 4c .. 4c + 3 and dpred receives its gradient there.  Every other element of
 * dpred - the other classes' columns, the pad columns, background rows - is written as exactly 0 by the same launch, whatever
 * it held.  All four kinds; SMOOTH_L1 takes any beta >= 0 (0 = plain L1, the gradient bits of u2_box_reg_l1).  An unknown
 * kind, beta < 0 or LP < 4 * bg_label returns -1; R == 0 launches nothing. */
int u2_box_reg_loss_cls(int kind, const void* pred, const float* prop, const float* gtb, const void* labels, void* dpred,
                        float* loss, int R, int LP, int bg_label, float wx, float wy, float ww, float wh, float beta,
                        float scale_clamp, float gscale, void* stream);

/* ---- ROI bookkeeping (roi.hip) -----------------------------------------------------------------
 * layers/roi_align.py:49-65 via modeling/poolers.py:206-263; structures/masks.py:191-218; modeling/poolers.py:23-59;
 * structures/boxes.py:312-358 + modeling/matcher.py:62-127; modeling/box_regression.py:78-116; layers/nms.py:9-20. */
/* `order` (may be NULL): a permutation of 0 .. R-1, the order the ROIs are PROCESSED in (results stay at their own rows of `out`):
 * with ROIs sorted by (level, image, row) the work-groups running at any one time read neighbouring feature rows, and each XCD
 * takes a contiguous part of the list, so its L2 keeps the band it is working on. */
int u2_roi_align_fwd(const void* const* feats, const int* Hs, const int* Ws, const float* scales, int nlevels,
                     const float* rois, const int* level, const int* order, void* out, int R, int C, int PH, int PW,
                     void* stream);
int u2_roi_align_bwd(float* const* gfeats, const int* Hs, const int* Ws, const float* scales, int nlevels,
                     const float* rois, const int* level, const void* dout, int R, int C, int PH, int PW, float gscale,
                     void* stream);
/* atomics-free backward: `order` lists ROI ids grouped by (image, level), seg[b*nlevels + l] .. seg[.. + 1] is the
 * group's range; gfeats[l] are bf16 NHWC gradient maps written in full (no pre-zeroing needed). */
int u2_roi_align_bwd_gather(void* const* gfeats, const int* Hs, const int* Ws, const float* scales, int nlevels,
                            const float* rois, const int* order, const int* seg, const void* dout, int B, int C, int PH,
                            int PW, float gscale, void* stream);
/* ROIs grouped by (image, level) for u2_roi_align_bwd_gather(_multi): order int32 [R] = ROI indices sorted by
 * key = image * nlevels + level with equal keys in index order (stable, = torch.argsort(key, stable=True)); seg int32
 * [num_images * nlevels + 1] = first position of every key, seg[last] = R.  rois [R][5] (image index first), level int32 [R].
 * num_images * nlevels <= 256, R <= 32768 and 512 * (num_images * nlevels + 2) + 2 * R <= 156 KB (the sort runs in one
 * work-group's LDS); -1 otherwise. */
int u2_roi_group(const float* rois, const int* level, int* order, int* seg, int R, int num_images, int nlevels, void* stream);
/* The same gather over up to four ROI sets at once (the cascade's three box poolers and the mask pooler share the FPN
 * maps): set i has its own rois / order / seg / dout, pooled size P[i] x P[i] and gradient scale.  Each level's gradient
 * map is written once; the per-set gradient maps and their sums (autograd's accumulation) are never formed. */
int u2_roi_align_bwd_gather_multi(void* const* gfeats, const int* Hs, const int* Ws, const float* scales, int nlevels,
                                  int nsets, const void* const* rois, const void* const* order, const void* const* seg,
                                  const void* const* dout, const int* P, const float* gscale, int B, int C, void* stream);
/* The same launch for the levels of `level_mask` only (bit l; gfeats[l] of the others may be NULL), with up to two more gradient
 * maps per level added in fp32 before the one bf16 rounding: add0[l] / add1[l] (NULL arrays or NULL entries: none) are bf16 maps of
 * gfeats[l]'s shape - the gradients the map's OTHER readers produced (RPN head, semantic head: meta_arch/panoptic_fpn.py:105-131),
 * i.e. autograd's accumulation over a tensor with several consumers happens where the last addend is formed. */
int u2_roi_align_bwd_gather_sum(void* const* gfeats, const int* Hs, const int* Ws, const float* scales, int nlevels,
                                int level_mask, int nsets, const void* const* rois, const void* const* order,
                                const void* const* seg, const void* const* dout, const int* P, const float* gscale,
                                const void* const* add0, const void* const* add1, int B, int C, void* stream);
int u2_mask_crop(const void* masks, const float* rois, void* out, int R, int H, int W, int P, void* stream);
/* The crops of a whole batch in one launch: image i's bitmaps are mask_bases[i] ([K_i][Hs[i]][Ws[i]] uint8, host arrays of
 * device pointers / sizes), roi_image[r] (device) is the image of ROI r, rois[r] = (bitmap row in that image, x0, y0, x1, y1). */
int u2_mask_crop_batch(const void* const* mask_bases, const int* Hs, const int* Ws, int n_images, const float* rois,
                       const int* roi_image, void* out, int R, int P, void* stream);
int u2_assign_levels(const float* boxes, int* level, int n, int min_level, int max_level, float canonical_size,
                     int canonical_level, void* stream);
int u2_iou_match(const float* boxes, int per_image_boxes, const float* gt, const int* ngt, int* match, float* mval,
                 unsigned int* gt_max, signed char* labels, int B, int n, int G, float lo, float hi,
                 int allow_low_quality, void* stream);
int u2_apply_deltas(const float* src, const float* deltas, const int* img, const float* sizes, float* out, int n,
                    float wx, float wy, float ww, float wh, float clamp, int do_clip, void* stream);
/* The class-specific decode (fast_rcnn.py:494-524): deltas [R][LP] (bf16 if deltas_bf16 else fp32) with 4 K valid columns, src
 * fp32 [R][4] -> out fp32 [R][4 K], class c of row r = u2_apply_deltas (no clip) of columns 4c .. 4c + 3 against src[r].  One
 * thread per (row, class); the source boxes are not repeated.  LP < 4 K returns -1. */
int u2_apply_deltas_cls(const float* src, const void* deltas, int deltas_bf16, float* out, int R, int K, int LP, float wx,
                        float wy, float ww, float wh, float clamp, void* stream);
long long u2_nms_workspace_bytes(int B, int n);
int u2_batched_nms(const float* boxes, const int* group, const int* cnt, void* workspace, int* keep, int* nkeep, int B,
                   int n, float thr, int max_keep, void* stream);

/* ---- selection with a total order (select.hip) -----------------------------------------------
 * proposal_generator/proposal_utils.py:79-96 (per-level pre-NMS topk on the objectness logits, the score sort in front of
 * batched_nms) and modeling/sampling.py:38-54 in its "k smallest random keys" form.  Every row is ranked by
 * (value descending if largest else ascending, index ascending) - torch.topk leaves the order of ties open.  Values compare
 * as in torch.sort: -0.0 equals +0.0 and every NaN (either sign, any payload) is the greatest value; out_vals reports them as
 * +0.0 and as the quiet NaN 0x7fc00000.
 *   vals: fp32 (dtype 0) or bf16 (dtype 1); element i of row r is vals[r * row_stride + (i / group) * pitch + i % group]
 *         (group = pitch = 1: contiguous rows; group = A, pitch = 32: the A valid columns of a 32-wide NHWC logit map);
 *   mask (optional, int8 [rows][n]): only elements with mask == mask_value take part;
 *   out_vals (optional) / out_idx [rows][k]: the k best in rank order; entries beyond out_cnt[r] = min(k, participants)
 *   are (-/+inf, 0).  n < 2^24, k <= 16384;
 *   idx_in (optional, int32 [rows][n], values in [0, 2^24)): the index element i stands for - ties are broken on it and it
 *   is what out_idx reports - so that the survivors of a first selection over segments of a long row can be merged by a
 *   second call with the same total order. */
int u2_topk_rows(const void* vals, int dtype, int rows, int n, long long row_stride, int group, int pitch,
                 const signed char* mask, int mask_value, int k, int largest, float* out_vals, int* out_idx,
                 int* out_cnt, const int* idx_in, void* stream);

/* Proposal decoding of all feature levels in one launch (proposal_generator/rpn.py:482-533, proposal_utils.py:56-91, the part
 * between the per-level top-k and the NMS): for level l and image b the k_l candidates idx[b][j] (anchor index = pixel * A + anchor,
 * ranked) with logits scores[b][j] are decoded from the NHWC bf16 deltas map (`deltas` points at channel 0 of the 4 A delta channels
 * of pixel 0, `pitch` channels per pixel) against anchors [hwa][4], clipped to sizes[b] = (h, w), and written as rows of kmax >= k_l:
 * boxes / scores [B * L][kmax] with row = b * L + l (padding: zero box, score -3e38), keep[row][j] = finite and wider / taller than
 * min_size; *nonfinite (pre-zeroed) counts candidates with a non-finite box or logit. */
typedef struct U2RpnLevel {
  const void* deltas;
  const float* anchors;
  const int* idx;
  const float* scores;
  int hwa, k, pitch, reserved;
} U2RpnLevel;
int u2_rpn_decode(const U2RpnLevel* levels, int L, int A, int B, int kmax, const float* sizes, float wx, float wy, float ww, float wh,
                  float clamp, float min_size, float* boxes, float* scores, signed char* keep, int* nonfinite, void* stream);

/* Several selections in one launch (up to 8 segments; a work-group per row of every segment): the per-level pre-NMS top-k of
 * proposal_utils.py:79-96 over all feature levels at once, or the positive and the negative draw of sampling.py:38-54 over the
 * same keys.  Fields as the arguments of u2_topk_rows, plus:
 *   cnt_in / cnt_group: element i takes part iff i % cnt_group < cnt_in[row * (n / cnt_group) + i / cnt_group] - the rows of a
 *     first selection (k entries each, cnt real ones) concatenated as the input of a merging second selection;
 *   idx_mod / idx_mul: the reported index is the element's index + (row % idx_mod) * idx_mul - rows that are equal segments of a
 *     longer row report positions in that row (idx_mod = 1, idx_mul = 0: none);
 *   dtype 2: fp32 storage of bf16-representable values (the fp32 out_vals of a first selection over a bf16 map): ranked on the
 *     upper 16 bits only. */
typedef struct U2TopkSeg {
  const void* vals;
  const signed char* mask;
  const int* idx_in;
  const int* cnt_in;
  float* out_vals;
  int* out_idx;
  int* out_cnt;
  long long row_stride;
  int dtype, rows, n, group, pitch, mask_value, k, largest;
  int cnt_group, idx_mod, idx_mul, reserved;
} U2TopkSeg;
int u2_topk_rows_multi(const U2TopkSeg* segs, int nseg, void* stream);

/* ---- inference tails (postprocess.hip) -------------------------------------------------------
 * layers/mask_ops.py:17-147 (paste_masks_in_image, GPU branch), meta_arch/panoptic_fpn.py:184-269. */
/* meta_arch/semantic_seg.py:240-244 + panoptic_fpn.py:173 at inference: logits [B][H][W][Cp] NHWC bf16 (K valid channels) ->
 * out (optional) fp32 NCHW [B][K][H*S][W*S] = F.interpolate(logits.float(), scale_factor=S, mode="bilinear",
 * align_corners=False) and argmax (optional) int64 [B][H*S][W*S] = out.argmax(1) (first maximum), one pass. */
int u2_semseg_upsample(const void* logits, float* out, long long* argmax, int B, int H, int W, int Cp, int K, int S,
                       void* stream);
/* modeling/postprocessing.py:77-100 (sem_seg_postprocess): the [C][Hin][Win] fp32 window of a larger map (channel stride in_cs,
 * row stride in_rs, in elements) -> out fp32 [C][Hout][Wout] = F.interpolate(window, size=(Hout, Wout), mode="bilinear",
 * align_corners=False): source index scale * (dst + 0.5) - 0.5 clamped at 0 with scale = in / out in fp32, like ATen. */
int u2_bilinear_resize_f32(const float* in, float* out, int C, int Hin, int Win, long long in_cs, long long in_rs, int Hout,
                           int Wout, void* stream);
/* out[k][y][x] (uint8 0/1) = bilinear sample of probs[k] (P x P fp32) on F.grid_sample(align_corners=False)'s grid over
 * boxes[k] = (x0, y0, x1, y1), zero outside the map, >= threshold.  `out` is 16-byte aligned. */
int u2_paste_masks(const float* probs, const float* boxes, void* out, int n, int P, int H, int W, float threshold,
                   void* stream);
/* mask_rcnn_inference (detectron2/modeling/roi_heads/mask_head.py:115-158) with the 1x1 predictor folded in: only the predicted
 * class's channel is formed.  x: bf16 [N][S2][S2][C] trunk output (C % 8 == 0, C <= 1024), or with phased = 1 the 2x2 / stride-2 deconvolution's
 * GEMM output before its pixel shuffle, [N][S2/2][S2/2][2][2][C]; Wp [K][C], bp [K] fp32 master parameters (rounded to bf16 like the
 * conv operands); cls int64 [N]; prob fp32 [N][S2][S2] = sigmoid(bf16(x . Wp[cls] + bp[cls])). */
int u2_mask_predict_prob(const void* x, const float* Wp, const float* bp, const void* cls, float* prob, int N, int S2, int C,
                         int phased, void* stream);
/* The same for the masks of a batch of images in one launch (detectron2/modeling/postprocessing.py:9-74 pastes per image):
 * image i owns rows [first, first + n) of probs / boxes and writes its n canvases of H x W bytes at byte out_offset (a multiple
 * of 16) of the 16-byte aligned `out` (the padding bytes between two images' canvases may be zeroed); `images` is a HOST array. */
typedef struct U2PasteImage { int first, n, H, W; long long out_offset; } U2PasteImage;
int u2_paste_masks_batch(const float* probs, const float* boxes, void* out, const U2PasteImage* images, int num_images, int P,
                         float threshold, void* stream);
/* Panoptic merge of a batch of images (one work-group each); `images` is a HOST array of descriptors holding device
 * pointers.  inst_segment[rank] = segment id given to the rank-th highest scoring instance (0 = rejected); stuff_segment /
 * stuff_area [num_sem] = id (0 = rejected) and free-pixel area per semantic label.  boxes (optional) + mask_res bound the
 * pixels a pasted mask can occupy (half a source texel past the box); boxes == NULL scans the whole image. */
typedef struct U2PanopticImage {
  const unsigned char* masks; /* [K][H][W] 0/1 */
  const int* order;           /* [K] instance index by descending score */
  const float* scores_sorted; /* [K] */
  const float* boxes;         /* [K][4] or NULL */
  const long long* semantic;  /* [H][W] argmax of the semantic head, rows sem_stride elements apart */
  int* panoptic;              /* [H][W] out */
  int* inst_segment;          /* [K] out */
  int* stuff_segment;         /* [num_sem] out */
  int* stuff_area;            /* [num_sem] out */
  int K, H, W, num_sem;
  int sem_stride;             /* >= W: the label map may be a window of a wider (padded) map */
} U2PanopticImage;
int u2_panoptic_merge(const U2PanopticImage* images, int n_images, float overlap_thr, int stuff_area_thr, float score_thr,
                      int mask_res, void* stream);

/* ---- mask evaluation (maskeval.hip): the "segm" task of evaluation/coco_evaluation.py, DESIGN.md section 11 -----------------
 * Bit planes: a mask of H x W is W columns of wpc = ceil(H / 64) 64-bit words, column-major like COCO's RLE scan: bit b of
 * word j of column x = pixel (y = 64 j + b, x), padding bits zero.  A ragged batch is described by a HOST array: image i owns
 * the per-mask entries [first, first + n) of area / box / offs, its n canvases of H x W bytes start at byte in_offset (a
 * multiple of 16) of the 16-byte aligned canvases, its n planes of W * wpc words at word plane_offset of `planes`, and its
 * n * W per-column entries at col_offset of colcnt / last3 / cntcum / lastne / collen / strcum.  H * W < 2^31, n <= 65535;
 * images with n, H or W == 0 are skipped.  All results are integers: exact. */
typedef struct U2MaskImage { int first, n, H, W; long long in_offset, plane_offset, col_offset; } U2MaskImage;
/* canvases (uint8, nonzero = set; what u2_paste_masks_batch writes) -> planes; every byte is read once (16-byte loads, a
 * 64-row band transposed through LDS).  area [M] (set pixels) and box [M][4] = x, y, w, h of the tight box (zeros for an
 * empty mask) are written when both are given. */
int u2_mask_pack_planes(const void* canvases, void* planes, int* area, int* box, const U2MaskImage* images, int num_images,
                        void* stream);
/* The COCO counts strings of the planes' masks, byte for byte data/rle.py's encode: count -> scan -> lengths -> scan -> emit.
 * u2_mask_rle_count: colcnt[col] = run starts (pixels that differ from their predecessor in the column-major scan, the
 * predecessor of pixel (0, 0) being 0) in that column, last3[col][3] = scan positions x H + y of its last three, newest first.
 * The caller then forms cntcum = inclusive prefix sum of colcnt and lastne[col] = the last col' <= col with colcnt > 0 (-1:
 * none), both over the flat column list.  u2_mask_rle_lengths: collen[col] = characters the column's counts take (the final
 * count of a mask belongs to its last column).  With strcum = inclusive prefix sum of collen, u2_mask_rle_emit writes the
 * characters of column col at arena[strcum[col - 1]...] (nothing at or past arena_bytes): the string of a mask is
 * arena[strcum[c0 - 1] : strcum[c0 + W - 1]) with c0 its first column. */
int u2_mask_rle_count(const void* planes, int* colcnt, int* last3, const U2MaskImage* images, int num_images, void* stream);
int u2_mask_rle_lengths(const void* planes, const int* colcnt, const int* last3, const long long* cntcum,
                        const long long* lastne, int* collen, const U2MaskImage* images, int num_images, void* stream);
int u2_mask_rle_emit(const void* planes, const int* colcnt, const int* last3, const long long* cntcum, const long long* lastne,
                     const long long* strcum, void* arena, long long arena_bytes, const U2MaskImage* images, int num_images,
                     void* stream);
/* Ground truth: uncompressed counts -> planes.  cum = inclusive prefix sums of the flat list of all masks' counts, offs
 * [M + 1] = index of every mask's first count (mask first + k of image i uses offs[first + k], offs[first + k + 1]); the counts
 * of a mask must sum to H * W (the caller checks).  Every word of the planes is written, padding included. */
int u2_mask_planes_from_counts(const long long* cum, const long long* offs, void* planes, const U2MaskImage* images,
                               int num_images, void* stream);
/* inter[out_offset + d * G + g] = popcount(dt plane d & gt plane g) for every image of the HOST array: its D detection planes
 * start at word dt_offset of dt_planes, its G ground-truth planes at word gt_offset of gt_planes, both H x W.  dt_boxes
 * (optional, [..][4] as written by u2_mask_pack_planes, the image's rows starting at dt_first) limits the words read to the
 * detection's columns.  D == 0 or G == 0: nothing is written. */
typedef struct U2PairImage { long long dt_offset, gt_offset, out_offset; int D, G, H, W, dt_first, pad_; } U2PairImage;
int u2_mask_pair_counts(const void* dt_planes, const void* gt_planes, const int* dt_boxes, int* inter,
                        const U2PairImage* images, int num_images, void* stream);
/* Ground truth: polygon annotations -> planes (polygon.hip), bit for bit data/polygon.py's
 * polygons_to_bitmask: cocoapi's rleFrPoly per polygon, the union over an annotation's polygons.  xy: device float64, the
 * vertices x0, y0, x1, y1, ... of all polygons; |5 x + .5| must stay below 2^31 (the caller checks).  poly_offs [P + 1]: device,
 * index of every polygon's first vertex; a polygon has at least one vertex.  masks: a HOST array, one entry per output mask:
 * its plane of W * ceil(H / 64) words at word plane_offset of `planes`, its polygons [first_poly, first_poly + num_polys).
 * Every word of every addressed plane is written, padding included (num_polys == 0: zeros); masks with H or W == 0 are skipped
 * and their area entry is left alone.  area [num_masks] (optional) = set pixels.  H * W < 2^31.  scratch: device words for the
 * toggle planes of every polygon after a mask's first (the first uses the mask's own plane): at least
 * u2_mask_polygon_scratch_words(masks, num_masks) = sum of (num_polys - 1) * W * ceil(H / 64) over the masks with num_polys > 1;
 * may be NULL when that is 0.  Integer XOR atomics and plain stores only: the result does not depend on any order. */
typedef struct U2PolyMask { int H, W; long long plane_offset; int first_poly, num_polys; } U2PolyMask;
long long u2_mask_polygon_scratch_words(const U2PolyMask* masks, int num_masks);
int u2_mask_planes_from_polygons(const double* xy, const long long* poly_offs, const U2PolyMask* masks, int num_masks,
                                 void* planes, int* area, void* scratch, long long scratch_words, void* stream);

/* ---- pseudo-panoptic label merge (labelprep.hip): data/pseudo_panoptic.py's merge_image, DESIGN.md section 18 ----------------
 * A ragged batch of images in a HOST array.  Image i: its n instances in paint order (rank 0 is painted first, rank n - 1
 * last and on top) as n planes of W * ceil(H / 64) words from word plane_offset of `planes` (the layout above, as
 * u2_mask_planes_from_counts writes it); its semantic labels, uint8 [H][W], from byte pix_offset of `sem` (0..26 are the 27
 * classes, any other value belongs to none); the same pix_offset, in elements, places the image in rank, label and ids, and
 * 3 * pix_offset in rgb.  pix_offset is a multiple of 4; first = instances of the images before it (its entries of
 * `present`).  H * W < 2^31, n <= 65535.  Integer atomics and plain stores only: no result depends on any order.
 * u2_label_paint: rank [pixels] = 1 + the highest rank whose plane has the pixel's bit (0: none); present [first + rank] = 1 for
 *   every rank that won a pixel, 0 otherwise; hist [num_images][U2_LABEL_HIST]: [c] = pixels of class c = label + 1 in 1..27,
 *   [32 + c] = those of them with rank != 0.  present and hist are cleared by the call.
 * u2_label_decide (one launch, the images in order): image i's instances are base_i + rank, base_0 = first_id (< 2^32);
 *   then every class c = 1..27 in order takes the next id iff hist[c] - hist[32 + c] > 0 and not 10 hist[32 + c] > 7 hist[c];
 *   base_(i+1) = the next free id.  counts [num_images] (device) = n of every image.  decisions [num_images][U2_LABEL_DEC]
 *   uint32: [l] = id of label l (0 = not claimed), [27] = next free id, [28] = base_i.  Ids are uint32 and must not pass 2^32
 *   (the caller checks first_id + sum(n + 27)).
 * u2_label_emit (each output optional): id = base_i + rank - 1 under an instance, else the label's id, else 0;
 *   rgb [pixels][3] uint8 = id & 255, id >> 8 & 255, id >> 16 & 255 (id2rgb, wrapping at 2^24 like it); label [pixels] uint8 = 0
 *   under an instance, c for a claimed class c, 255 elsewhere; ids [pixels] uint32 = id.  rank and ids 16-byte, sem, rgb and
 *   label 4-byte aligned. */
#define U2_LABEL_CLASSES 27
#define U2_LABEL_HIST 64
#define U2_LABEL_DEC 32
typedef struct U2LabelImage { int first, n, H, W; long long plane_offset, pix_offset; } U2LabelImage;
int u2_label_paint(const void* planes, const void* sem, int* rank, int* present, int* hist, const U2LabelImage* images,
                   int num_images, void* stream);
int u2_label_decide(const int* hist, const int* counts, void* decisions, long long first_id, int num_images, void* stream);
int u2_label_emit(const int* rank, const void* sem, const void* decisions, void* rgb, void* label, void* ids,
                  const U2LabelImage* images, int num_images, void* stream);

/* ---- panoptic quality (panopticeval.hip): evaluation/panoptic_ops.py, DESIGN.md section 12 ------------------------------------
 * The joint histogram PQ is computed from: for every image of the HOST array, counts[(G + 2)][P] = pixels shared by a
 * ground-truth row and a predicted id.  pred: the [H][W] int32 id map u2_panoptic_merge writes (0 = void), P = its largest
 * segment id + 1.  gt: the ground-truth png's pixels [H][W][3] uint8, id = R + 256 G + 65536 B formed on the device, or with
 * gt_is_ids = 1 an [H][W] int32 id map.  gt_table [G]: the ids of the ground truth's segments_info, strictly ascending.  Row 0 =
 * ground-truth id 0 (void), rows 1..G = the table's ids in order, row G + 1 = every id the table does not list.  A pixel whose
 * predicted id is < 0 or >= P enters no row and is counted in out_of_range[image] instead.  pred and gt must be 16-byte
 * aligned (the image is read as one flat run of pixels: rows need no alignment, the last partial piece is read pixel by
 * pixel, nothing past H * W pixels is touched); counts and out_of_range need no initialisation.  H * W < 2^31,
 * (G + 2) * P < 2^31.  A table of at most u2_panoptic_pair_lds_ints() entries is accumulated in LDS per work-group and folded
 * into counts, a larger one straight in counts; integer atomics either way: exact. */
typedef struct U2PanopticPairImage {
  const int* pred;           /* [H][W] */
  const void* gt;            /* [H][W][3] uint8, or [H][W] int32 with gt_is_ids */
  const int* gt_table;       /* [G] ascending (may be NULL when G == 0) */
  int* counts;               /* [(G + 2)][P] out */
  int H, W, G, P;
  int gt_is_ids, pad_;
} U2PanopticPairImage;
int u2_panoptic_pair_counts(const U2PanopticPairImage* images, int n_images, int* out_of_range, void* stream);
int u2_panoptic_pair_lds_ints(void);

/* ---- COCO AP matching and accumulation (cocoeval.hip): evaluation/cocoeval_ops.py, DESIGN.md section 15 -------------------------
 * The two stages of COCOeval the reference runs in C++ (layers/csrc/cocoeval/cocoeval.cpp), value for value what
 * evaluation/cocoeval.py's _match_image and accumulate compute.  Work is organised by cell = an (image, category) pair with at
 * least one ground truth or one detection; cells are ordered by (category, image position), so that the detections of a
 * category are one contiguous run of the flat detection arrays.  All pointers of the problem are device pointers.
 *   cell_dt_off / cell_gt_off / cell_iou_off [n_cells + 1]: first detection / ground truth / IoU entry of every cell; a
 *     cell's detections are in descending score order (stable), cut to the largest budget; its IoU table is [D'][G].
 *   dt_area: what the area ranges test (box area, or mask area in the mask form); dt_box / gt_box: xywh float64.
 *   mask form: IoU of (d, g) from inter[dt_row[d] + gt_col[g]], dt_marea[d], gt_marea[g] (int64 pixel counts).
 *   gt_crowd: a crowd region (ignored; its union is the detection's area; it can be matched repeatedly).
 *   perm [n_dt]: position in the flat detection arrays of every entry of the categories' lists, each list in descending score
 *     order (stable: image position, then rank); cat_dt_off [K + 1] delimits the lists.
 *   area_rng [A][2], iou_thrs [T], rec_thrs [R], max_dets [M]: the parameters, as the host holds them.
 * A * T <= 40, A <= 8, R <= 256, max_rank (largest D' of any cell) < 2^23.
 * u2_cocoeval_match: IoU tables, per-area ground-truth order and the greedy matching, one wave per cell; a cell with more
 * than u2_cocoeval_lds_iou_entries() IoU entries or more than u2_cocoeval_lds_max_gt() ground truth keeps its table and its
 * taken-flags in global memory.  rec_match / rec_ignore (both or neither; [n_dt][A * T]): matched column of the cell's
 * ground truth + 1 (0: none) and the detection-ignored flag.  u2_cocoeval_accumulate (after it, same workspace): precision and
 * scores [T][R][K][A][M], recall [T][K][A][M], every entry written; integer scans in chunks of u2_cocoeval_scan_chunk().
 * workspace: u2_cocoeval_workspace_bytes() bytes, 16-byte aligned, no initialisation; u2_cocoeval_workspace_layout also gives
 * the byte offsets of its parts: [0] IoU tables float64, [1] per-detection flag words, [2] the same in list order, [3] scores
 * in list order, [4] ground-truth order int32 [cell][A][G], [5] ground-truth ignored uint8 [cell][A][G] in that order,
 * [6] not-ignored ground truth per (category, area) int32, [7] taken-flags, [8] not-ignored ground truth per (cell, area)
 * int32, [9] path of every cell uint8 (0 = LDS, 1 = global memory).  It does not grow with T * A * M. */
typedef struct U2CocoEvalProblem {
  const long long* cell_dt_off;
  const long long* cell_gt_off;
  const long long* cell_iou_off;
  const int* cell_cat;
  const double* dt_area;
  const double* dt_score;
  const double* dt_box;
  const long long* dt_row;
  const long long* dt_marea;
  const double* gt_area;
  const double* gt_box;
  const unsigned char* gt_crowd;
  const long long* gt_col;
  const long long* gt_marea;
  const long long* inter;
  const int* perm;
  const long long* cat_dt_off;
  const double* area_rng;
  const double* iou_thrs;
  const double* rec_thrs;
  const int* max_dets;
  long long n_cells, n_dt, n_gt, iou_entries;
  int K, A, T, R, M, mask_form, max_rank, pad_;
} U2CocoEvalProblem;
long long u2_cocoeval_workspace_bytes(long long n_dt, long long n_gt, long long iou_entries, long long n_cells, int K, int A,
                                      int T);
long long u2_cocoeval_workspace_layout(long long n_dt, long long n_gt, long long iou_entries, long long n_cells, int K, int A,
                                       int T, long long* offsets /* host [10] */);
int u2_cocoeval_match(const U2CocoEvalProblem* problem, void* workspace, long long workspace_bytes, int* rec_match,
                      unsigned char* rec_ignore, void* stream);
int u2_cocoeval_accumulate(const U2CocoEvalProblem* problem, void* workspace, long long workspace_bytes, double* precision,
                           double* scores, double* recall, void* stream);
int u2_cocoeval_lds_iou_entries(void);
int u2_cocoeval_lds_max_gt(void);
int u2_cocoeval_scan_chunk(void);

/* ---- boundary IoU of the semantic evaluation (semeval.hip): evaluation/semseg_ops.py, DESIGN.md section 16 ---------------------
 * The reference's _mask_to_boundary (evaluation/sem_seg_evaluation.py:396-407) and the two bincounts of its process():
 * erode(m)[y][x] = minimum of m over the (2 d + 1) x (2 d + 1) window centred on (y, x), everything outside the image counted
 * as 0 (the zero ring and d passes of a 3 x 3 minimum); boundary(m) = m - erode(m) in uint8, a difference of label values.
 * pred, gt: [h][w] uint8 device maps, any alignment; lut: 256 uint8 entries applied to pred BEFORE the erosion, or NULL for
 * identity; d >= 1 is computed by the caller (max(1, round(0.02 * sqrt(h^2 + w^2))), half to even).  n <= 32 is the side of
 * the matrices; a pixel whose mapped prediction or ground truth is >= n is counted in neither.
 *   bconf[n * boundary(lut[pred]) + boundary(gt)] += 1 for every pixel, and, when conf is not NULL, from the same read
 *   conf[n * lut[pred] + gt] += 1.  Both are int64 [n][n] on the device, added to with integer atomics, never cleared: exact.
 * d <= u2_semseg_boundary_fused_cap(): one fused kernel (64 x 64 tile + halo in LDS), no scratch.  A larger d takes a row
 * pass and a column pass through scratch, u2_semseg_boundary_scratch_bytes(h, w, d) bytes owned by the caller (0 in the
 * fused range).  h * w < 2^31.  Returns -1 for n outside 1..32, d < 1, h or w < 1, a NULL map or bconf, or too little scratch. */
int u2_semseg_boundary_confusion(const void* pred, const void* gt, const void* lut, int h, int w, int d, int n,
                                 long long* conf, long long* bconf, void* scratch, long long scratch_bytes, void* stream);
int u2_semseg_boundary_fused_cap(void);
long long u2_semseg_boundary_scratch_bytes(int h, int w, int d);

/* ---- training augmentation on the device (augment.hip): data/device_mapper.py, DESIGN.md section 17 --------------------------
 * What the host mapper does with PIL and numpy after loading a sample - bilinear resize of the image, nearest resize of the
 * label map, RLE decode + nearest resize of the masks, flips - from tables the worker built on the host.  Everything is
 * integer arithmetic: exact.  One call per stage serves a whole per-GPU batch: `images` is a HOST array of descriptors.
 *
 * `block` is one device allocation of block_bytes bytes that holds every input of the batch, `tables_host` a host copy of the
 * same bytes (the pinned staging block it was copied from); the launchers read the tables and run ends of the host copy to
 * check the contract before anything is launched, the kernels read the device copy.  Offsets named *_offset are byte offsets
 * into the block, the table fields are int32 ELEMENT offsets into it (block and every table 4-byte aligned):
 *   bx_bounds [W][2] / by_bounds [H][2]: (first source index, tap count >= 1) per output index, first + count <= w / h,
 *   count <= kx / ky;  bx_coef [W][kx] / by_coef [H][ky]: int32 coefficients (22 fractional bits);
 *   nx [W] / ny [H]: nearest source index per output index;
 *   mask_offs [num_masks + 1]: where every mask's run ends begin (and the last one's end), as elements behind ends_base (itself
 *   an element offset into the block); a mask's run ends are the inclusive prefix sums of its RLE counts, uint32:
 *   non-decreasing, at least one, the last one == h * w.
 * A flip is a reversed table: the kernels know nothing about it.  x_identity / y_identity: w == W / h == H, that pass is
 * skipped (its table has one tap and is used as an index table only).  row0, nrows: the source rows the vertical pass reads
 * (every by_bounds row inside [row0, row0 + nrows)); only those go through the horizontal pass.  h * w and H * W < 2^31.
 * Status: 0 ok; -1 bad argument (sizes, offsets or buffers too small); -2 bad run ends; -3 a table entry out of range.  Nothing
 * is launched and no output is written unless the status is 0. */
typedef struct U2AugImage {
  int h, w, H, W;
  int kx, ky, x_identity, y_identity;
  int row0, nrows, num_masks, first_mask;
  long long src_offset, lab_offset;              /* HWC uint8 [h][w][3]; uint8 [h][w] (-1: no label map) */
  long long img_out_offset, lab_out_offset, mask_out_offset; /* bytes in img_out; int64 ELEMENTS in lab_out; bytes in mask_out */
  long long bx_bounds, bx_coef, by_bounds, by_coef, nx, ny, mask_offs, ends_base;
} U2AugImage;
/* img_out[img_out_offset + (c * H + y) * W + x] = clip8((2^21 + sum_k t[c][by_first[y] + k][x] * by_coef[y][k]) >> 22) with
 * t[c][r][x] = clip8((2^21 + sum_k src[r][bx_first[x] + k][c] * bx_coef[x][k]) >> 22) rounded to uint8 (PIL's order: horizontal
 * first), any tap count.  scratch: u2_aug_resize_bilinear_scratch_bytes(images, num_images) bytes (t of the images that
 * need both passes; -1 for a bad descriptor). */
long long u2_aug_resize_bilinear_scratch_bytes(const U2AugImage* images, int num_images);
int u2_aug_resize_bilinear_u8(const void* block, long long block_bytes, const void* tables_host, void* img_out,
                              long long img_out_bytes, void* scratch, long long scratch_bytes, const U2AugImage* images,
                              int num_images, void* stream);
/* lab_out[lab_out_offset + y * W + x] = label[ny[y]][nx[x]] as int64; images with lab_offset < 0 are skipped. */
int u2_aug_resize_nearest_u8(const void* block, long long block_bytes, const void* tables_host, long long* lab_out,
                             long long lab_out_elems, const U2AugImage* images, int num_images, void* stream);
/* mask_out[mask_out_offset + (m * H + y) * W + x] = parity of the number of run ends of mask m that are <= nx[x] * h + ny[y]
 * (bytes 0 / 1), counts[first_mask + m] = the number of 1 bytes written (int32, cleared by the call). */
int u2_aug_rle_masks(const void* block, long long block_bytes, const void* tables_host, void* mask_out,
                     long long mask_out_bytes, int* counts, int num_counts, const U2AugImage* images, int num_images,
                     void* stream);
/* The same decode through a window of a larger annotation (INPUT.CROP), with the tight box of what was
 * written.  windows: HOST array, one per image.  Mask m of image i is a run-length code over mask_h x mask_w, column-major;
 * the descriptor's (h, w) is the size of the window, its nx / ny index the window, and output pixel (y, x) reads position
 * p = (x0 + nx[x]) * mask_h + y0 + ny[y].  mask_out and counts as above.  boxes: int32 [num_counts][4] on the device,
 * boxes[first_mask + m] = (min x, min y, max x + 1, max y + 1) over the 1 bytes written, (0, 0, 0, 0) when there are none;
 * cleared by the call.  Integer min / max only: no result depends on an order.  The walk's waves send atomic minima / maxima
 * (the maxima with the + 1) into boxes preset to (INT_MAX, INT_MAX, 0, 0); a short second kernel on the same stream then zeroes
 * the boxes of the masks without a pixel - a second pass, not an encoding.
 * Checked on the host before anything is launched (status -1, for the run ends -2): x0, y0 >= 0, x0 + w <= mask_w,
 * y0 + h <= mask_h, mask_h * mask_w < 2^31, every mask's last run end == mask_h * mask_w, boxes not NULL where there are masks.
 * With the window (0, 0, h, w) mask_out and counts are those of u2_aug_rle_masks. */
typedef struct U2AugWindow { int x0, y0, mask_h, mask_w; } U2AugWindow;
int u2_aug_rle_masks_boxes(const void* block, long long block_bytes, const void* tables_host, void* mask_out,
                           long long mask_out_bytes, int* counts, int* boxes, int num_counts, const U2AugImage* images,
                           const U2AugWindow* windows, int num_images, void* stream);

/* ---- optimizer (optim.hip): solver/build.py:36-37,63-73,119-139 ------------------------------- */
int u2_sgd_clip_step(float* params, const float* grads, float* momentum_buf, const int* chunk_tensor,
                     const long long* chunk_begin, const int* chunk_len, int n_chunks, float* partial /*[n_chunks]*/,
                     const int* tensor_first_chunk /*[n_tensors + 1]*/, const float* wd_per_tensor, float lr, float momentum,
                     float clip, float grad_scale, void* stream);
/* The same step with the solver's other options (solver/build.py:29-46 CLIP_TYPE / NORM_TYPE, :130-139 NESTEROV, :187-199
 * BIAS_LR_FACTOR); u2_sgd_clip_step is what the default configuration keeps calling.  The arithmetic restates torch's, fp32:
 *   norm pass (clip_mode 2, 3, 4 only): partial[c] = sum g^2 (2: L2), sum |g| (3: L1) or max |g| (4: inf) over chunk c, 1024
 *     threads and float4 over head / body / tail as in the L2 pass, which IS that of u2_sgd_clip_step; sums in a fixed order,
 *     no atomics, so every data-parallel rank forms the same coefficient.  Per tensor t: total = sqrt(sum) (2), sum (3) or
 *     max (4) of its partials, times grad_scale;  coef = min(clip / (total + 1e-6f), 1)  - clip_grad_norm_(p, clip, norm_type),
 *     per parameter.
 *   step pass (always one launch), per element:
 *     g' = g (coef grad_scale)                        clip_mode 2, 3, 4
 *     g' = clamp(g grad_scale, -clip, +clip)          clip_mode 1: clip_grad_value_(p, clip) on the averaged gradient
 *     g' = g grad_scale                               clip_mode 0
 *     d = g' + wd[t] p;   m' = momentum m + d;   u = nesterov ? d + momentum m' : m';   p' = p - lr_t u,
 *     lr_t = lr_class_per_tensor[t] ? lr_bias : lr    (the two rates a yacs config can form: BASE_LR, BASE_LR BIAS_LR_FACTOR)
 *   A zero-filled momentum arena gives torch's first-step rule buf = d, with Nesterov too (u = d + momentum d, as torch).
 *   Non-finite gradients: the inf norm's fmaxf drops a NaN where torch's max propagates it (the clamp of mode 1 keeps it).
 * clip_mode outside 0..4, or a clip <= 0 with clip_mode != 0, is refused (-1): "no clipping" is mode 0. */
int u2_sgd_step_opts(float* params, const float* grads, float* momentum_buf, const int* chunk_tensor,
                     const long long* chunk_begin, const int* chunk_len, int n_chunks, float* partial /*[n_chunks]*/,
                     const int* tensor_first_chunk /*[n_tensors + 1]*/, const float* wd_per_tensor,
                     const int* lr_class_per_tensor /* 0: lr, 1: lr_bias */, float lr, float lr_bias, float momentum,
                     int nesterov, int clip_mode /* 0 none, 1 value, 2 L2, 3 L1, 4 inf */, float clip, float grad_scale,
                     void* stream);

/* ---- k-means over DINO embeddings (kmeans.hip): u2seg/Instance_Clustering/shared/utils/nn_utils.py:304-379 ---- */
/* labels[i] = argmin_j |x_i - c_j|^2 (first minimum).  workspace: u2_kmeans_assign_workspace_floats(N, D, K) floats (contents
 * need no initialisation; keep the same buffer between the iterations of a run: it also carries the screening state).  The
 * distances are screened on bf16 MFMA - first with the leading bf16 piece of x and c alone, then, for the points that pass
 * cannot decide, with the split products hi.hi + hi.lo + lo.hi - and every point whose two best candidates are closer than
 * the screening error bound is labelled again with exact fp32 products, so the result is that of the exact kernel
 * (exact_only = 1 runs only that one; it is also what D % 32 != 0 or K > 320 fall back to).  After the call
 * ((int*)workspace)[((K + 3) & ~3) + 1] holds the number of points re-checked exactly, [... + 2] the number the first pass
 * left undecided. */
long long u2_kmeans_assign_workspace_floats(int N, int D, int K);
int u2_kmeans_assign(const float* x, const float* c, float* workspace, long long* labels, int N, int D, int K, int exact_only,
                     void* stream);
/* The same with a shadow of x: x does not change between the Lloyd iterations of a run (nn_utils.py:352 builds its x_i once,
 * outside the loop), so u2_kmeans_prepare writes mu = the column mean of x, fp16(S (x - mu)) with a power-of-two scale S (argmin_j
 * |x - c_j|^2 does not change under a common translation, and the screening margin is proportional to the norms of what is
 * multiplied; fp16 has the MFMA rate of bf16 and three more bits), the norm of x - mu, the norm of what the rounding dropped and |x_p|
 * once -
 * u2_kmeans_shadow_floats(N, D) floats, 0 when D % 32 != 0 - and the first screening pass of every later E step streams 2 instead
 * of 4 bytes per element, with a margin per point from those norms instead of a worst case.  Labels are the exact kernel's either way;
 * shadow = NULL: u2_kmeans_assign (first pass on bf16(x), rounded on the fly).  With a shadow the
 * screening also serves 320 < K <= 1280 (one first pass per block of 320 centroids, then the exact kernel for the undecided points;
 * [... + 1] counts those, [... + 2] is not written); without one such K run the exact kernel alone.
 * The shadow must be re-made when x changes. */
long long u2_kmeans_shadow_floats(int N, int D);
int u2_kmeans_prepare(const float* x, float* shadow, int N, int D, void* stream);
int u2_kmeans_assign_shadow(const float* x, const float* shadow, const float* c, float* workspace, long long* labels, int N, int D,
                            int K, int exact_only, void* stream);
/* csum [K][D] += sum of the rows of x by label, counts [K] += label histogram (both pre-zeroed by the caller, or holding
 * another shard's partial sums).  workspace (optional, u2_kmeans_update_workspace_floats(N, D, K) floats): the points are
 * bucketed by label there and the sums become a segmented reduction that reads every row of x once, whole (0.75 -> ~4 TB/s);
 * without it, or with D > 2048, a privatised-LDS kernel is used.  In both forms a label outside [0, K) (tested as int64) belongs to
 * no cluster.  Returns -1 and launches nothing for a K no form serves (K > 16384 with a workspace, K > 2168 without); N <= 0: 0.
 * u2_kmeans_finalize: c = csum / counts elementwise (an empty cluster: 0 / 0 = NaN, as in the reference). */
long long u2_kmeans_update_workspace_floats(int N, int D, int K);
int u2_kmeans_update(const float* x, const long long* labels, float* csum, float* counts, int N, int D, int K,
                     float* workspace, void* stream);
int u2_kmeans_finalize(const float* csum, const float* counts, float* c, int D, int K, void* stream);

/* ---- k nearest neighbours over the same embeddings (knn.hip): nn_utils.py:204-299 (kNN, partitioned_kNN) ----
 * d_knn[i][0..K) = the K smallest sum_d (x_query[i][d] - x_train[j][d])^2 in ascending order (ties: smaller j first),
 * ind_knn[i][k] = the train row j it belongs to; what pykeops' Kmin_argKmin(K, dim=1) returns at nn_utils.py:216 and what
 * partitioned_kNN's merge over 130 000-row partitions (:226-266) reduces to.  D % 16 == 0, 1 <= K <= 28, Nt >= K (else -2).
 * workspace: u2_knn_workspace_ints() 4-byte words of device memory. */
int u2_knn_workspace_ints(int Nq, int Nt, int D, int K, long long* n_ints);
int u2_knn(const float* x_query, const float* x_train, void* workspace, float* d_knn /*[Nq][K]*/,
           long long* ind_knn /*[Nq][K]*/, int Nq, int Nt, int D, int K, void* stream);

/* ---- USL selection regularizer (usl.hip): nn_utils_imagenet.py:147-212 (get_selection_with_reg_imagenet's update) -------
 * For every row i of x [N][D]: the H smallest sum_d (x[i][d] - sel[j][d])^2 over the S rows of sel [S][D] (ties: smaller j),
 * masked (exclude_same_cluster != 0: 1e10 where the position j == labels[i]; else 1e10 where the distance is 0), then
 * new = sum 1 / v (alpha == 1) or sum 1 / v ** alpha, and reg_out[i] = reg_in[i] * momentum + new * one_minus_momentum.
 * Rows that keep a 0 after the mask add 1 to *zero_count (device int, zeroed by the caller): the reference's
 * AssertionError.  D % 16 == 0, 1 <= H <= 64, S >= H (else -2); N == 0 is a no-op.
 * workspace: u2_usl_reg_workspace_ints() 4-byte words of device memory. */
int u2_usl_reg_workspace_ints(int N, int S, int D, int H, long long* n_ints);
int u2_usl_regularizer(const float* x, const float* sel, const long long* labels, const float* reg_in, float* reg_out,
                       int* zero_count, void* workspace, int N, int S, int D, int H, float alpha, float momentum,
                       float one_minus_momentum, int exclude_same_cluster, void* stream);

/* ---- DINO ViT instance features (vit.hip): u2seg/Instance_Clustering/selective_labeling/dino.py:77-308 --------------------
 * Stage 1's feature extractor (ViTFeat.forward, dino.py:296-308).  The linears (qkv, proj, fc1, fc2, patch_embed.proj) run
 * through u2_conv_igemm; these kernels do the rest.  bf16 = raw uint16 bits; the residual stream is fp32 [B][T][D].
 *
 * Patch rows for patch_embed.proj (dino.py:170-173): out bf16 [B * P][3 * patch * patch], P = (H / patch) * (W / patch) in
 * row-major grid order, columns in (c, kh, kw) order (the weight [D][3][p][p] viewed as [D][3 p p]).  in_u8 = 1: img is
 * uint8 NHWC RGB [B][H][W][3] and norm device fp32 [6] = mean[3], std[3]: (u / 255 - mean) / std in fp32, torchvision's
 * ToTensor + Normalize (shared/utils/nn_utils_imagenet.py:411-430); in_u8 = 0: img is fp32 NCHW already normalised
 * (norm may be NULL).  C must be 3. */
int u2_vit_patchify(const void* img, const float* norm, void* out, int B, int H, int W, int C, int patch, int in_u8,
                    void* stream);
/* prepare_tokens (dino.py:224-235): x[b][0] = cls[:] + pos[0], x[b][1 + p] = (patch_out[b * (T - 1) + p] + bias) + pos[1 + p],
 * all adds in fp32; patch_out is the bf16 GEMM output [B * (T - 1)][out_ld] without its bias, pos fp32 [T][D]. */
int u2_vit_embed(const void* patch_out, int out_ld, const float* bias, const float* cls, const float* pos, float* x,
                 int B, int T, int D, void* stream);
/* Block.forward's residual add and the next LayerNorm (dino.py:135-142, 281/292 LayerNorm(eps)), one pass per row:
 * row r of the residual is x + r * x_stride; if branch != NULL: x += branch[r * branch_stride] (bf16) + branch_bias (fp32,
 * may be NULL), written back; then out[r * out_stride] = LayerNorm(x) with fp32 statistics (biased variance), bf16, or fp32
 * when out_fp32 (the final norm; dino.py:304-308).  D % 64 == 0, D <= 1024.  x_stride = T * D visits only the CLS rows. */
int u2_vit_residual_layernorm(float* x, long long x_stride, const void* branch, long long branch_stride,
                              const float* branch_bias, const float* gamma, const float* beta, void* out,
                              long long out_stride, int out_fp32, int rows, int D, float eps, void* stream);
/* Attention.forward (dino.py:108-120) without the attention matrix: q, k, v of (image b, token t, head h, d) are columns
 * s * D + h * 64 + d (s = 0, 1, 2) of qkv row b * T + t (qkv_ld elements per row, D = heads * 64: reshape(B, N, 3, H, C/H));
 * out bf16 [B][q_rows][D], column h * 64 + d: (softmax(q k^T * head_dim^-0.5) v).transpose(1, 2).reshape(B, N, C) for the
 * first q_rows queries of every image (q_rows = T, or 1 for the CLS row alone).  bf16 operands, fp32 accumulation and
 * softmax.  head_dim must be 64; qkv 16-byte aligned, qkv_ld % 8 == 0. */
int u2_vit_attention(const void* qkv, void* out, int B, int T, int heads, int head_dim, int qkv_ld, int q_rows, void* stream);
/* nn.GELU() (exact erf form, dino.py:77-93) in place on n bf16 elements (n % 8 == 0, 16-byte aligned). */
int u2_vit_gelu(void* x, long long n, void* stream);

/* ---- test-time augmentation for instance inference (tta.hip): detectron2/modeling/test_time_augmentation.py:244-307 ---------
 * The box maps between a view (resized, possibly flipped) and the original image, and the mean of the views' mask
 * probabilities, for the views of ALL images of a call in one launch each (modeling/test_time_augmentation.py, DESIGN.md
 * section 19).  The arithmetic is the reference's numpy float32 arithmetic, one rounding per step.
 *
 * A view v is described by view_desc[v] = (s1x, s1y, s2x, s2y, width) (float32), view_flip[v] (0 / 1) and view_image[v] (the
 * image it belongs to).  Every array is device memory; boxes are [.][4] float32 (x0, y0, x1, y1), 16-byte aligned.
 * Status: 0 ok, -1 a bad argument (nothing launched).  Zero rows, zero views of an image and views without rows are valid.
 *
 * View -> original (TransformList.inverse().apply_box): if flip, (x0, x1) = minmax(width - x0, width - x1); then x * s1x * s2x and
 * y * s1y * s2y (two multiplications; 1.0f where a step is absent); after every step the box is the min / max of its mapped
 * corners as numpy takes them (a NaN in x0 or x1 makes both NaN).  row_view[i]: the view of row i.  out_cand[i] (uint8) = all
 * four mapped coordinates finite and scores[i] finite and scores[i] > score_thresh; out_boxes[i] = the mapped box clipped to
 * [0, image_clip[image][0]] x [0, image_clip[image][1]] (width, height) like Boxes.clip (a NaN stays a NaN). */
int u2_tta_boxes_to_original(const float* boxes, const float* scores, const int* row_view, const float* view_desc,
                             const int* view_flip, const int* view_image, const float* image_clip, float* out_boxes,
                             void* out_cand, int num_rows, int num_views, int num_images, float score_thresh, void* stream);
/* Original -> view (TransformList.apply_box): x * s1x * s2x, y * s1y * s2y, then the flip; not clipped.  The boxes of image i
 * are rows image_rows[i] .. image_rows[i + 1] (int32 [num_images + 1]); view v writes them to rows view_out_row[v] .. of out.
 * max_rows: the largest row count of an image. */
int u2_tta_boxes_to_views(const float* boxes, const int* image_rows, const float* view_desc, const int* view_flip,
                          const int* view_image, const long long* view_out_row, float* out, int max_rows, int num_views,
                          int num_images, void* stream);
/* out[image_rows[i] + r][0][y][x] = (sum over the views v = image_views[i] .. image_views[i + 1] - 1, in this order, of
 * view_prob[v][r][0][y][view_flip[v] ? P - 1 - x : x]) / float(number of views): sequential float32 additions, one division.
 * view_prob: device array of num_views pointers to float32 [rows of the image][1][P][P].  max_rows as above; min_views: the
 * smallest view count of an image (>= 1). */
int u2_tta_reduce_masks(const void* view_prob, const int* view_flip, const int* image_views, const int* image_rows, float* out,
                        int max_rows, int min_views, int num_images, int P, void* stream);
/* The mean of the views' semantic logits of ONE image, n views per call:
 *   acc[c][y][x] = (sum over the views v of all calls, in order, of term_v[c][y][flip_v ? W - 1 - x : x]) / float(divisor)
 * with term_v = sem_seg_postprocess(view v's [C][h_v][w_v] window, (h_v, w_v), H, W): u2_bilinear_resize_f32's value in its
 * arithmetic, or the source element itself when (h_v, w_v) == (H, W), so that a NaN or an Inf passes through as it does there.
 * Sequential float32 additions in view order, one division: the views of an image split over calls in any grouping that
 * keeps their order give the same bits as one call.
 *   view_logits  DEVICE array of n pointers to float32 logits (the window's element [0][0][0]; x stride 1)
 *   views        HOST array [n][5]: h, w, row stride, channel stride (in elements), flip (0 / 1)
 *   acc          float32 [C][H][W], in / out; first != 0: the sum starts from the first view's term, acc is not read
 *   divisor      > 0: this is the last call, every element is divided by float(divisor) after the additions; 0: not yet
 *   argmax       optional int64 [H][W], written on the last call only: the first maximum over c, a NaN counting as the largest
 * Status: 0 ok; -1 (nothing launched) for C < 1, C > 64, n < 1, H or W < 1, a window side < 1, a row stride below the window's
 * width, a negative channel stride or divisor, a null view_logits, views or acc. */
int u2_tta_accumulate_sem_seg(const void* view_logits, const long long* views, int n, float* acc, int first, int divisor,
                              long long* argmax, int C, int H, int W, void* stream);

/* library self-description */
int u2_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
