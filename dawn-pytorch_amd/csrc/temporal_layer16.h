// Geometry of the window-tiled fused temporal layer (temporal_layer16.hip), shared with its launcher's schedule and with the LDS bank
// model (tools/tl16_lds_banks.cpp): the byte offsets below are the ones the kernels use, so model and kernels cannot drift.
#pragma once
#define TL16_WAVES 8           /* 2 per SIMD: 256 registers each -- every weight fragment of a stage is requested a stage ahead */
#define TL16_ROWS 208          /* row slots of the X / K planes (a multiple of 16: the plane stride is a multiple of 256 B, so the k-groups of a ds_read_b128 fragment read -- lanes {n, n + 16} with disjoint n per lane group -- fall on disjoint banks) */
#define TL16_KEY_BLOCKS 6      /* 16-key blocks per 16-query tile: 16 + 2 win <= 96 */
#define TL16_LDS_BYTES 161856  /* X planes 79,872 + K planes 39,936 + V^T 39,936 + bias table copies 2,112 */
#define TL16_BAND_ROOM 132     /* floats reserved per shifted bias-table copy (the LDS size above counts 4 of them) */
#define TL16_BAND_STRIDE 112   /* floats between the copies in use: 48 mod 64 banks = 12 of the 16 four-bank quads.  A ds_read_b128 lane group
                                  reads twelve distinct 16-byte pieces, three per copy: at this stride they land on twelve different quads (a
                                  stride of 4 mod 64 -- 132 -- put three of them on one quad: 3-way, +8 LDS cycles per read; 0 mod 64 -- 128 --
                                  four).  tools/tl16_lds_banks.cpp prices every stride that fits. */
#define TL16_BAND_ENTRIES 108  /* entries of a copy that are ever read: 12 + 12 + 16 . 5 + 3 is the last */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TL16_HD __host__ __device__
#else
#define TL16_HD
#endif

// ---- LDS regions of the fused kernels, in bytes from the start of dynamic LDS (the attention core keeps K, V^T and the table only)
constexpr int TL16_X_BYTES = 3 * 8 * TL16_ROWS * 16;
constexpr int TL16_K_BYTES = 3 * 4 * TL16_ROWS * 16;
constexpr int TL16_BLOCKS = TL16_ROWS / 16;                 // 16-row blocks
constexpr int TL16_V_BYTES = 3 * TL16_BLOCKS * 2 * 512;
constexpr int TL16_BAND_BYTES = 4 * TL16_BAND_ROOM * 4;
constexpr int TL16_X_BASE = 0, TL16_K_BASE = TL16_X_BYTES, TL16_V_BASE = TL16_K_BASE + TL16_K_BYTES, TL16_BAND_BASE = TL16_V_BASE + TL16_V_BYTES;
static_assert(TL16_BAND_BASE + TL16_BAND_BYTES == TL16_LDS_BYTES, "LDS layout");
static_assert(4 * TL16_BAND_STRIDE <= 4 * TL16_BAND_ROOM && TL16_BAND_ENTRIES <= TL16_BAND_STRIDE, "bias table copies");

// ---- byte offsets inside a region
// X planes [plane 3][channel octet 8][row] x 16 B (two 8-byte halves: channels 8 o + 4 half + r)
TL16_HD constexpr int tl16_x_off(int plane, int octet, int row, int half) { return ((plane * 8 + octet) * TL16_ROWS + row) * 16 + half * 8; }
// K planes [plane 3][k-group 4][row] x 16 B (half = 16-feature half of the head)
TL16_HD constexpr int tl16_k_off(int plane, int g, int row, int half) { return ((plane * 4 + g) * TL16_ROWS + row) * 16 + half * 8; }
// V^T [plane 3][m-block 2][lane 64][row block 13] x 8 B
TL16_HD constexpr int tl16_v_off(int plane, int mb, int lane, int blk) { return (((plane * 2 + mb) * 64 + lane) * TL16_BLOCKS + blk) * 8; }
// bias table: float index of entry e of shifted copy sh; and of the float4 that lane (query n, k-group g) adds to slot `blk` of its S^T
TL16_HD constexpr int tl16_band_idx(int sh, int e) { return sh * TL16_BAND_STRIDE + e; }
TL16_HD constexpr int tl16_band_read_idx(int n, int g, int blk) { return tl16_band_idx((15 - n) & 3, ((15 - n) & ~3) + 4 * g + 16 * blk); }

