// kargs.h -- kernel argument blocks and host-side launcher prototypes shared by the translation units.
#pragma once
#include "common.h"
#include <atomic>
#include <type_traits>
#include <mutex>

struct ConvArgs {
    const int8_t *x;
    const int8_t *wp;
    const int32_t *cw, *dzp, *bias;
    const double *mval, *sval;
    uint8_t *y;
    int32_t *acc_out;
    float *y_f32;
    int in_cs, in_lead, in_cells;
    int out_cs, out_lead;
    int out_w, pool_w;       // bytes of an output / pooled cell this layer may write (16-aligned channel count)
    int B, H, W, n;          // H, W: input map
    int stride, OH, OW;      // output map = (H + 2*pad - ksize) / stride + 1 (== H, W for the stride-1 kernels)
    int ksize, cb, nchunks, upc, spc, ksteps;
    int total_n, ntiles_n, mtiles;
    int xcd_mb;              // conv_rows: tiles are numbered in blocks of xcd_mb M tiles, N-major inside a block (1 = M-major): what one XCD's contiguous range covers
    // conv_rows: launch constants of the index arithmetic (divisions by them are multiplications, common.h FastDiv)
    FastDiv fd_hw, fd_w, fd_ntn, fd_ntper, fd_nch, fd_mb;  // H * W, W, ntiles_n, xcd_mb * ntiles_n, channel chunks, xcd_mb
    int tile_q, tile_r;      // N tile t covers pixels [t q + min(t, r), + q + (t < r))
    int zp_act, act, store_mode;
    float s_act;
    int mpad;
    int bchunks, bpt;        // LDS B buffer size in KiB chunks; DMA instructions per wave per chunk load
    int tiles_x, tiles_y;    // PATCH mode tiling of one image
    int rows_cap;            // conv_rows: LDS rows per B buffer
    int rowb;                // conv_rows: bytes between LDS rows (row data + bank skew)
    const int32_t *shift;    // per-channel right shift (valid when hdr->pow2)
    const double *mprime;    // M_value * shift_value
    const int32_t *cwb;      // cw + bias
    const ConvBlobHeader *hdr;
    uint8_t *ypool;          // fused 2x2/2 maxpool output (PHWC, biased) or null
    int pool_cs, pool_lead;
    int lds_param_off;       // conv_rows: byte offset of the staged per-channel epilogue parameters in LDS
    int debug;               // timing-ablation switches (results are wrong when non-zero): see mi355_debug_flags
    const int8_t *ws;        // conv_small: weights-stationary A fragments [m-tile][k-step][lane][16 B] or null
    int sm_ncell, sm_pieceb; // conv_small: slots (16 B per piece plane) per LDS image row = its pitch; bytes of one 16-channel piece plane
    int sm_lcell, sm_hc;     // conv_small: image cells per row (<= sm_ncell) and the slot of the row's first ODD cell: a row holds its even
                             // cells 0, 2, .. in slots 0 .., its odd cells in slots sm_hc .. (see conv_small.hip: conflict-free stride-2 reads)
    int sm_tp;               // conv_mid_pool: pooled pixels per tile
    int sm_nq, sm_red_off;   // conv_ws3: filter quads (waves) per K part and workgroup; LDS offset of the K-part partial sums
    int pool_mode;           // conv_ws3: 0 = none, 2 = fused 2x2 / stride-2 maxpool (ypool = the pooled map), 1 = fused 2x2 / stride-1
                             // maxpool (ypool = a map of the conv's own size; ref: pad = 1 -> window rows y..y+1, columns x..x+1, clipped)
    int sm_pt_off, sm_pt_stride;  // conv_ws3: LDS offset / slot stride of the staged output bytes the fused pool reads
    int up;                  // conv_rows: fused nearest-neighbour upsample factor of the stored tensor (1 = none)
    float *yolo_out;         // fused yolo head: activated copy of y_f32 (same layout) or null
    int yolo_per;            // classes + 5
    // fused quantized residual add (mi355_conv_shortcut_forward): the stored byte is shortcut(conv byte, res byte); res is
    // the `from` layer's tensor, same map as y.  res_delta = (res.lead - y.lead): res cell = y cell + res_delta
    const uint8_t *res;
    int res_cs, res_delta;
    int sc_ka, sc_kb, sc_k0;
    int plan;                // MI355_PLAN_*: throughput plan = prefer kernels of which two workgroups fit a CU
    const EptHeader *ept;    // the blob's epilogue table (common.h) or null
};

struct AuxArgs {
    const uint8_t *x;  // input tensor (cs==4: plain uint8 image cells; else biased PHWC)
    int in_cs, in_lead, in_cells;
    const uint32_t *wfirst;  // first-layer packing [n][9] dwords
    const uint8_t *w_u8;     // raw reference weights [n][c*k*k] (ref-f32 kernel)
    const uint8_t *zp_w;     // [n]
    const int32_t *dzp, *bias;
    const double *mval, *sval;
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int B, H, W, c, n, ksize, pad;
    int zp_in, zp_act, act, store_mode;
    float s_act;
    int total_n;
    const double *mprime;    // folded M_value * shift_value
    uint8_t *ypool;          // fused 2x2/2 maxpool output or null
    int pool_cs, pool_lead;
    const ConvBlobHeader *hdr;  // device copy of the blob header (data-dependent pow2 flag)
    const int32_t *cwb;         // cw + bias (first-layer MFMA kernel)
    int planar;                 // x is the reference's [B][3][H][W] uint8 planes (no cells, no pads), read in place
    int debug_flags;            // mi355_debug_flags (2048: plain tile walk instead of the XCD-aware one, A/B runs)
    const EptHeader *ept;       // the blob's epilogue table (common.h) or null
    FastDiv fd_tpi, fd_tx;      // first-layer MFMA kernels: divisions by tiles per image / tiles per row
    // per-image input quantisation (mi355_conv_forward_per_image): the blob pointers above are entry 0 of a bank of entries
    // `entry_bytes` apart; image b uses entry entry_of_image[b] and the input zero point zp_of_image[b] (zp_in is unused).
    // Read only by the kernels' PI instantiations.
    const int32_t *entry_of_image;
    const uint8_t *zp_of_image;
    long entry_bytes;
    int pi_wpi;                 // first-layer MFMA kernels, PI: workgroups per image (a workgroup walks the tiles of one image)
};

// The view of a per-image bank that image b sees: every per-entry pointer moved to entry entry_of_image[b], the image's own
// input zero point.  Identity for the shared-scale instantiations (PI = false).  The packed weights are the same in every
// entry (one layer, packed for different input scales), so kernels that stage them before knowing the image use entry 0's.
template <bool PI>
__device__ __forceinline__ std::conditional_t<PI, AuxArgs, const AuxArgs &> bank_entry(const AuxArgs &a, int b)
{
    if constexpr (!PI) {
        return a;
    } else {
        AuxArgs e = a;
        const long off = (long)a.entry_of_image[b] * a.entry_bytes;
        auto mv = [off](auto *p) { return p ? reinterpret_cast<decltype(p)>(reinterpret_cast<const char *>(p) + off) : p; };
        e.wfirst = mv(a.wfirst); e.dzp = mv(a.dzp); e.bias = mv(a.bias);
        e.mval = mv(a.mval); e.sval = mv(a.sval); e.mprime = mv(a.mprime);
        e.hdr = mv(a.hdr); e.cwb = mv(a.cwb); e.ept = mv(a.ept);
        e.zp_in = a.zp_of_image[b];
        return e;
    }
}

struct PoolArgs {
    const uint8_t *x;
    uint8_t *y;
    int B, H, W, OH, OW, cs_in, cs_out, in_lead, out_lead, groups;  // groups = C/16
    int size, stride, offset;                                       // offset = -pad/2
};

struct CopyArgs {
    const uint8_t *x;
    uint8_t *y;
    int B, H, W, OH, OW, cs_in, cs_out, in_lead, out_lead, groups, stride, coff;  // coff: channel offset in y
};

struct DequantArgs {
    const uint8_t *t;
    float *out;
    int B, H, W, cs, lead, c0, nc, out_C, out_c0, zp;
    float scale;
};

struct ShortcutArgs {
    const uint8_t *a, *b;
    uint8_t *y;
    int B, H, W, groups;
    int a_cs, b_cs, y_cs, a_lead, b_lead, y_lead;
    int ka, kb, k0;
};

struct LayoutArgs {
    uint8_t *nchw;
    uint8_t *t;
    int B, H, W, C, cs, lead;
};

// conv_kxk.hip: the general-shape convolution (any size 1..11, stride, padding, channel count) and its ref-f32 twin
struct KxkArgs {
    const uint8_t *x;        // input tensor: cs == 4 plain image cells, else biased PHWC (cs % 16 == 0)
    int in_cs, in_lead;
    int B, H, W, c;          // input map and channels
    int n, ksize, stride, pad, OH, OW;
    const int8_t *wk;        // packed A fragments [mpad / 32][ksteps][64 lanes][16 B] (ConvBlobHeader.generic)
    int unit, nchunks, spc, ksteps;  // K layout: unit = channel bytes per tap (4 | 8 | 16), spc = K-steps per channel chunk
    const int32_t *cw, *dzp, *bias, *cwb;
    const double *mval, *sval, *mprime;
    const ConvBlobHeader *hdr;  // device copy (pow2 flag)
    const uint8_t *w_u8, *zp_w; // ref-f32 kernel: raw reference weights [n][c k k], zero points
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_in, zp_act, act, store_mode;
    float s_act;
    int tw_sh, tiles_x, tiles_y, mgroups, ph, pw;  // tile geometry (set by the launcher)
};
int conv_kxk_launch(KxkArgs &a, hipStream_t st);
int conv_ref_f32_general_launch(KxkArgs &a, hipStream_t st);
// K of the general kernel is (channel chunk, tap, channel in the chunk) with `unit` channel bytes per tap: few-channel layers pack 4 or 8
// channels of a tap densely (the 3-channel image: 4-byte cells), the others 16-channel chunks (the last one padded with zero weights)
inline int kxk_unit(int c) { return c <= 4 ? 4 : (c <= 8 ? 8 : 16); }
struct KxkGeom { int unit, nchunks, spc, ksteps, mpad; };
inline KxkGeom kxk_geom(int n, int c, int ksize)
{
    KxkGeom g;
    g.unit = kxk_unit(c);
    const int tpl = 16 / g.unit;                      // taps per 16-byte lane fragment
    g.nchunks = g.unit == 16 ? (c + 15) / 16 : 1;
    g.spc = (ksize * ksize + 2 * tpl - 1) / (2 * tpl);  // K-steps per chunk: 2 lane halves of tpl taps each
    g.ksteps = g.nchunks * g.spc;
    g.mpad = ((n + 127) / 128) * 128;                 // rows padded to the largest M tile
    return g;
}

// conv_dw.hip: the depthwise convolution (groups == c == n).  Its blob (mi355_conv_dw_pack) is a header and per-channel arrays padded to
// whole 64-channel chunks, offsets a function of (c, ksize) only:
//     wd      int16 [c64 / 64][ksize * ksize][64]   w_u8 - zp_w of (chunk, tap, channel in the chunk); 0 for channels >= c
//     bias    int32 [c64]      mval, sval, mprime   f64 [c64]   (mprime = M_value * shift_value, common.h requant_q_exact)
#define MI355_DW_MAGIC 0x4D494457u /* "MIDW" */
struct DwBlobHeader {
    uint32_t magic;
    int32_t c, ksize, c64;
    int32_t pow2;        // 1: every shift_value is an exact power of two (ConvBlobHeader.pow2)
    int32_t pad_[3];
    uint64_t off_wd, off_bias, off_mval, off_sval, off_mprime, total;
};
inline bool dw_blob_layout(int c, int ksize, DwBlobHeader *h)
{
    if (c < 1 || ksize < 1 || ksize > 11) return false;
    *h = DwBlobHeader{};
    h->magic = MI355_DW_MAGIC; h->c = c; h->ksize = ksize; h->c64 = (c + 63) / 64 * 64;
    uint64_t off = (sizeof(DwBlobHeader) + 15) & ~(uint64_t)15;
    h->off_wd = off;     off += (uint64_t)h->c64 * ksize * ksize * 2;
    off = (off + 15) & ~(uint64_t)15;
    h->off_bias = off;   off += (uint64_t)h->c64 * 4;
    h->off_mval = off;   off += (uint64_t)h->c64 * 8;
    h->off_sval = off;   off += (uint64_t)h->c64 * 8;
    h->off_mprime = off; off += (uint64_t)h->c64 * 8;
    h->total = off;
    return true;
}
struct DwArgs {
    const uint8_t *x;        // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W, c;          // input map; channels == filters
    int ksize, stride, pad, OH, OW;
    const int16_t *wd;
    const int32_t *bias;
    const double *mval, *sval, *mprime;
    const DwBlobHeader *hdr; // device copy (pow2 flag)
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_in, zp_act, act, store_mode;
    float s_act;
    int plan;
    // tile geometry (set by the launcher)
    int ry_sh;               // the 16 pixel runs of a workgroup are 2^ry_sh rows by 16 >> ry_sh runs
    int tiles_x, tiles_y, nchunks;
    int ph, pw, pitch;       // staged patch: rows, cells per row, LDS cells between rows (odd)
    int pieces16;            // 16-byte pieces of a cell that hold channels: ceil(c / 16)
    FastDiv fd_pw;
};
constexpr int DW_RUN = 8;    // output pixels along x per lane; the tile is 2^ry_sh rows by (16 >> ry_sh) * DW_RUN columns
int conv_dw_launch(DwArgs &a, hipStream_t st);  // MI355_EINVAL when no tile fits LDS (nothing launched)

// conv_sep.hip: the depthwise-separable block: a depthwise layer (its mi355_conv_dw_pack blob) and the dense 1x1
// layer that reads it (its mi355_conv_pack blob) in one launch; the intermediate tensor stays in LDS
struct SepArgs {
    const uint8_t *x;        // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W, c;          // input map; channels == depthwise filters == the 1x1 layer's channels
    int ksize, stride, pad, OH, OW;  // the depthwise layer's; OH x OW is also the 1x1 layer's map
    // depthwise stage (DwBlobHeader's arrays)
    const int16_t *wd;
    const int32_t *dbias;
    const double *dmval, *dsval, *dmprime;
    const DwBlobHeader *dhdr;  // device copy: compared with the launch, and the pow2 flag
    int zp_in, zp_mid, dact, dstore;  // zp_mid: the depthwise layer's zp_act = the 1x1 layer's zp_in
    // pointwise stage (ConvBlobHeader's arrays)
    int n;
    const int8_t *wk;        // gen: general-kernel A fragments [mpad / 32][ksteps][64 lanes][16 B]; else the row plane [mpad / 16][ksteps][4][16 rows][16 B]
    int gen, cb_sh, ksteps;  // cb_sh: log2 of the row plane's 16-channel units per K-step (cb / 16)
    int mt32;                // 32-row tiles the plane holds: mpad / 32
    const int32_t *cw, *dzp, *bias;
    const double *mval, *sval, *mprime;
    const ConvBlobHeader *hdr;  // device copy: compared with the launch, and the pow2 flag
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_act, act, store_mode;
    float s_act;
    int plan;
    // tile geometry (set by the launcher): conv_dw.hip's tile and patch, and this kernel's buffers
    int ry_sh, tiles_x, tiles_y, nchunks;
    int ph, pw, pitch, pieces16;
    int pbytes, pbufs;       // bytes of one patch buffer (patch, then the runtime-size path's weights); patch buffers: 1 | 2
    int fblocks;             // filter blocks of 128 (n <= SEP_FILTERS_MS1) or 256 filters: the depthwise stage is recomputed per block
    FastDiv fd_pw;
};
constexpr int SEP_FILTERS_MS1 = 128;  // up to here a wave owns 32 filters (64 accumulator registers), above 64 (128)
int conv_sep_launch(SepArgs &a, hipStream_t st);  // MI355_EINVAL when no tile fits LDS (nothing launched)

// conv_tr.hip: the transposed convolution ([deconvolutional]), split into its stride x stride output phases.  Phase
// (ty, tx) owns the taps ky = ty + s jy, kx = tx + s jx, numbered t = jy * tr_taps(k, s, tx) + jx.  With nu = ceil(c / 16) channel
// units, a phase's K-steps (32 bytes: two lane halves of one unit of one tap) are dense: first (unit pair up, tap t) -> step
// up * taps + t with half kh on unit 2 up + kh; then, for an odd nu, the last unit's taps in pairs -> half kh on tap 2 tp + kh.
// The blob (mi355_conv_tr_pack) is a header, the A fragments [phase][mpad / 32][steps of the phase][64 lanes][16 B], per-filter
// arrays and two int32 per (phase, filter): cw = 128 sum w' + 128 d K_phase over the phase's own taps, and sw = sum (w - zp_w) over
// every other tap, which the kernel multiplies by the input zero point (the stuffed cells of the dense twin).
#define MI355_TR_MAGIC 0x4D495452u /* "MITR" */
constexpr int TR_MAX_STRIDE = 8;
constexpr int TR_MAX_TAPS = 128;   // tap slots of the kernel's offset table (11 x 11 at stride 1: 121)
__host__ __device__ inline int tr_taps(int k, int s, int t) { return t < k ? (k - t + s - 1) / s : 0; }
__host__ __device__ inline int tr_steps(int nu, int taps) { return (nu / 2) * taps + ((nu & 1) ? (taps + 1) / 2 : 0); }
struct TrBlobHeader {
    uint32_t magic;
    int32_t n, c, ksize, stride, mpad, nu;
    int32_t step0[TR_MAX_STRIDE * TR_MAX_STRIDE + 1];  // K-steps of the phases before phase ty * s + tx (per 32-row M tile)
    uint64_t off_wk, off_cw, off_sw, off_dzp, off_bias, off_mval, off_sval, total;
};
inline bool tr_blob_layout(int n, int c, int ksize, int stride, TrBlobHeader *h)
{
    if (n < 1 || c < 1 || ksize < 1 || ksize > 11 || stride < 1 || stride > TR_MAX_STRIDE) return false;
    *h = TrBlobHeader{};
    h->magic = MI355_TR_MAGIC; h->n = n; h->c = c; h->ksize = ksize; h->stride = stride;
    h->mpad = (n + 127) / 128 * 128;  // rows padded to the largest M tile
    h->nu = (c + 15) / 16;
    int steps = 0;
    for (int ph = 0; ph < stride * stride; ++ph) {
        h->step0[ph] = steps;
        steps += tr_steps(h->nu, tr_taps(ksize, stride, ph / stride) * tr_taps(ksize, stride, ph % stride));
    }
    h->step0[stride * stride] = steps;
    uint64_t off = (sizeof(TrBlobHeader) + 15) & ~(uint64_t)15;
    h->off_wk = off;   off += (uint64_t)(h->mpad / 32) * steps * 64 * 16;
    h->off_cw = off;   off += (uint64_t)stride * stride * h->mpad * 4;
    h->off_sw = off;   off += (uint64_t)stride * stride * h->mpad * 4;
    h->off_dzp = off;  off += (uint64_t)h->mpad * 4;
    h->off_bias = off; off += (uint64_t)h->mpad * 4;
    h->off_mval = off; off += (uint64_t)h->mpad * 8;
    h->off_sval = off; off += (uint64_t)h->mpad * 8;
    h->total = off;
    return true;
}
struct TrArgs {
    const uint8_t *x;        // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W, c;
    int n, ksize, stride, pad, OH, OW;
    const int8_t *wk;
    const int32_t *cw, *sw, *dzp, *bias;
    const double *mval, *sval;
    const TrBlobHeader *hdr; // device copy (step0)
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_in, zp_act, act, store_mode;
    float s_act;
    int plan;
    // tile geometry (set by the launcher).  A tile is 2^tw_sh columns of quotient space: output (oy, ox) of phase (ty, tx) sits at
    // (qy, qx) = ((oy + pad) / s, (ox + pad) / s), and tap (jy, jx) reads input (qy - jy, qx - jx)
    int nu, mpad, halo;      // halo = ceil(k / s) - 1 input rows / columns before the tile
    int tw_sh, tiles_x, tiles_y, mgroups, ph, pw;
    int cu, nchunks;         // channel units staged at a time (all of them when nchunks == 1; else even)
};
int conv_tr_launch(TrArgs &a, hipStream_t st);  // MI355_EINVAL when the grid does not fit (nothing launched)

// conv_group.hip: the grouped convolution (1 <= groups) as a block-diagonal GEMM on V_MFMA_I32_16X16X64_I8.  M tile t
// holds filters 16 t .. 16 t + 15; filter j belongs to group j / ng and reads channels [(j / ng) cg, (j / ng + 1) cg).  A PIECE is
// one 16-byte run of 16 channels of a cell; a SLOT is (piece, tap), one 16-lane group of a K-step.  A tile's K is cut into SEGMENTS
// at group boundaries: groups join a segment while its piece range stays within GRP_SEG_PIECES, a larger group is a segment alone.
// A segment's slots are (piece p0 + i, tap t) -> slot i k k + t, padded to whole K-steps with slots that point at (p0, tap 0)
// against zero weights.  Rows whose group lies outside the segment are zero in it, so a piece shared by two segments counts once.
// The blob (mi355_conv_group_pack) is a function of (n, c, groups, ksize) alone:
//     tseg    int32 [mtiles + 1]   first segment of each tile
//     seg     GrpSeg [nsegs]
//     frag    per segment: slot table int32 [4 nsteps] (piece - p0) << 8 | tap, then per K-step the weight fragment and the
//             indicator fragment (1 where the row's weight is live), each [64 lanes][16 B] in MFMA lane order
//     rows    GrpRow [16 mtiles]   per filter: d = 128 - zp_w, cst = 128 sum w' + 128 K d, the bias and the epilogue's multipliers
#define MI355_GRP_MAGIC 0x4D494752u /* "MIGR" */
constexpr int GRP_SEG_PIECES = 16;
constexpr int GRP_MAX_TAPS = 128;  // tap slots of the kernel's offset table (11 x 11: 121)
struct GrpSeg {
    int32_t tile, p0, npieces, nsteps;
    int32_t first, last;     // first / last segment of its tile: clear the accumulators / run the epilogue
    uint32_t off16;          // slot table, then fragments: 16-byte units from off_frag
    int32_t qa;              // first group of the segment (the last follows from the walk in grp_tile_segs)
};
struct GrpRow {
    int32_t d, cst, bias, pad_;
    double mval, sval, mprime;  // mprime = M_value * shift_value (common.h requant_q_exact)
};
struct GrpBlobHeader {
    uint32_t magic;
    int32_t n, c, groups, ksize, mtiles, nsegs;
    int32_t pow2;            // 1: every shift_value is an exact power of two (ConvBlobHeader.pow2)
    uint64_t off_tseg, off_seg, off_frag, off_rows, total;
};
inline bool grp_domain(int n, int c, int g, int ksize) { return n >= 1 && c >= 1 && g >= 1 && c % g == 0 && n % g == 0 && ksize >= 1 && ksize <= 11; }
// the segments of M tile t: piece range [p0, p0 + np) and group range [qa, qb] each; returns their number (at most 16)
inline int grp_tile_segs(int n, int c, int g, int t, int *p0, int *np, int *qa, int *qb)
{
    const int cg = c / g, ng = n / g;
    const int ga = 16 * t / ng, gb = (16 * t + 15 < n ? 16 * t + 15 : n - 1) / ng;
    int cnt = 0;
    for (int a = ga; a <= gb; ++cnt) {
        const int first = (int)((long)a * cg / 16);
        int b = a;
        while (b + 1 <= gb && (int)(((long)(b + 2) * cg - 1) / 16) - first + 1 <= GRP_SEG_PIECES) ++b;
        p0[cnt] = first; np[cnt] = (int)(((long)(b + 1) * cg - 1) / 16) - first + 1; qa[cnt] = a; qb[cnt] = b;
        a = b + 1;
    }
    return cnt;
}
inline bool grp_blob_layout(int n, int c, int g, int ksize, GrpBlobHeader *h)
{
    if (!grp_domain(n, c, g, ksize)) return false;
    *h = GrpBlobHeader{};
    h->magic = MI355_GRP_MAGIC; h->n = n; h->c = c; h->groups = g; h->ksize = ksize; h->mtiles = (n + 15) / 16;
    uint64_t frag = 0;
    int p0[16], np[16], qa[16], qb[16];
    for (int t = 0; t < h->mtiles; ++t) {
        const int ns = grp_tile_segs(n, c, g, t, p0, np, qa, qb);
        h->nsegs += ns;
        for (int i = 0; i < ns; ++i) {
            const uint64_t nsteps = ((uint64_t)np[i] * ksize * ksize + 3) / 4;
            frag += nsteps * (16 + 2048);
        }
    }
    if (frag / 16 > 0xFFFFFFFFull) return false;
    const uint64_t rows = (uint64_t)h->mtiles * 16;
    uint64_t off = (sizeof(GrpBlobHeader) + 15) & ~(uint64_t)15;
    h->off_tseg = off;   off = (off + ((uint64_t)h->mtiles + 1) * 4 + 15) & ~(uint64_t)15;
    h->off_seg = off;    off += (uint64_t)h->nsegs * sizeof(GrpSeg);
    h->off_frag = off;   off += frag;
    h->off_rows = off;   off += rows * sizeof(GrpRow);
    h->total = off;
    return true;
}
struct GrpArgs {
    const uint8_t *x;        // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W, c;
    int n, groups, ksize, stride, pad, OH, OW;
    const int32_t *tseg;
    const GrpSeg *seg;
    const char *frag;
    const GrpRow *rows;
    const GrpBlobHeader *hdr; // device copy (pow2 flag)
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_in, zp_act, act, store_mode;
    float s_act;
    int plan;
    // tile geometry (set by the launcher)
    int mtiles, mb, fblocks; // M tiles, M tiles per filter block, filter blocks
    int tw_sh, tiles_x, tiles_y, ph, pw;
    int plane;               // LDS cells between the planes of two pieces (odd)
    int restage;             // 1: a segment's pieces are staged when it is walked (the block's pieces do not fit together)
};
int conv_group_launch(GrpArgs &a, hipStream_t st);  // MI355_EINVAL when no tile fits LDS (nothing launched)

// conv_dil.hip: the dilated (atrous) stride-1 convolution as d x d dense convolutions on the phase-subsampled maps.
// Output (oy, ox) has phase (oy % d, ox % d) and phase index (oy / d, ox / d); tap (ky, kx) of it reads input
// (oy - pad + ky d, ox - pad + kx d), which is cell (jy + ky, jx + kx) of a patch gathered at cell stride d.  The A operand is the
// dense layer's: the general-kernel fragments of mi355_conv_pack (ConvBlobHeader.off_gen, K layout kxk_geom).
struct DilArgs {
    const uint8_t *x;        // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W, c;
    int n, ksize, dil, pad, OH, OW;
    const int8_t *wk;        // packed A fragments [mpad / 32][ksteps][64 lanes][16 B]
    int unit, nchunks, spc, ksteps;
    const int32_t *cw, *dzp, *bias;
    const double *mval, *sval, *mprime;
    const ConvBlobHeader *hdr;  // device copy (pow2 flag)
    uint8_t *y;
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_in, zp_act, act, store_mode;
    float s_act;
    // tile geometry (set by the launcher).  A phase tile is 2^th_sh x 2^tw_sh phase indices; a workgroup owns `slots` consecutive
    // tiles of the image's list [phase (qy, qx)][tile (ty, tx)], each with its own staged patch of ph x pw cells
    int th_sh, tw_sh, slots;
    int nqx, tiles_x, tpp, ntiles;  // phases along x: min(d, OW); tiles of a phase along x; tiles of a phase; tiles of an image
    int wpi, mgroups;           // workgroups per image and M group: ceil(ntiles / slots)
    int ph, pw;
    FastDiv fd_pc, fd_pw, fd_tpp, fd_tx, fd_nqx;  // patch cells, patch width, tiles per phase, tiles_x, nqx
};
int conv_dil_launch(DilArgs &a, hipStream_t st);  // MI355_EINVAL when no tile fits LDS (nothing launched)

// classify.hip: the fully connected layer as a skinny GEMM on V_MFMA_I32_16X16X64_I8 whose N dimension is the images.
// The K axis is "packed K": the input tensor's cell order, cell (y, x) after cell, cp = round_up(C, 16) bytes a cell (the 16-byte
// pieces of a cell that hold channels), Kp = H W cp, cut into K-steps of 64 bytes.  The tensor's own cell size may be larger (a window
// of a route's buffer): the kernel gathers cp bytes of every cell at the tensor's stride, so the blob (mi355_connected_pack) is a
// function of (n, C, H, W) alone and fits every cs % 16 == 0 that holds C:
//     frag    [mtiles][nsteps][64 lanes][16 B]: lane (m, q) of a step holds bytes 64 step + 16 q .. + 15 of filter 16 tile + m as
//             w - 128; byte kp is channel kp % cp of cell kp / cp, i.e. the reference's weight (kp % cp) H W + kp / cp, and 0 on the
//             spare channels C .. cp, past the last cell and in the rows past n
//     rows    GrpRow [16 mtiles]   per filter: d = 128 - zp_w, cst = 128 sum w' + 128 K d (K = C H W), bias, the epilogue's multipliers
#define MI355_FC_MAGIC 0x4D494643u /* "MIFC" */
constexpr int FC_MB = 4;               // M tiles (waves) of a workgroup
constexpr int FC_THREADS = 64 * FC_MB;
constexpr int FC_LDS_MAX = 64 * 1024;  // staged bytes of a chunk, every image of the group
constexpr int FC_MAX_K = 33024;        // K 255^2 < 2^31
constexpr int FC_CUS = 256;            // workgroups the launcher tries to reach by splitting K
constexpr int FC_MIN_STEPS = 8;        // K-steps of the shortest slice the rule makes
struct FcBlobHeader {
    uint32_t magic;
    int32_t n, C, H, W, cp, mtiles, nsteps;  // cp: packed bytes a cell, round_up(C, 16)
    int32_t pad_[2];
    uint64_t off_frag, off_rows, total;
};
inline bool fc_blob_layout(int n, int C, int H, int W, int cs, FcBlobHeader *h)
{
    if (n < 1 || C < 1 || H < 1 || W < 1 || cs % 16 || cs < C || (long)C * H * W > FC_MAX_K || (long)H * W * cs > (1L << 24)) return false;
    *h = FcBlobHeader{};
    h->magic = MI355_FC_MAGIC; h->n = n; h->C = C; h->H = H; h->W = W; h->cp = (C + 15) / 16 * 16;
    h->mtiles = (n + 15) / 16; h->nsteps = (H * W * h->cp + 63) / 64;
    h->off_frag = (sizeof(FcBlobHeader) + 15) & ~(uint64_t)15;
    h->off_rows = h->off_frag + (uint64_t)h->mtiles * h->nsteps * 1024;
    h->total = h->off_rows + (uint64_t)h->mtiles * 16 * sizeof(GrpRow);
    return true;
}
// split-K rule, a function of (n, K, B) alone: slices of at least FC_MIN_STEPS K-steps of the TRUE K until the grid reaches FC_CUS
// workgroups.  The launcher cuts the packed K-steps (>= the true ones) into that many slices of equal length and drops empty ones,
// so the rule's S bounds the launch's.
inline int fc_split(int n, int K, int B)
{
    const int base = (((n + 15) / 16 + FC_MB - 1) / FC_MB) * ((B + 63) / 64);
    const int most = ((K + 63) / 64) / FC_MIN_STEPS;
    int s = FC_CUS / base;
    if (s > most) s = most;
    return s < 1 ? 1 : s;
}
struct FcArgs {
    const uint8_t *x;        // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W, C;
    int n, ktrue, nsteps, cp;
    const FcBlobHeader *hdr; // device copy: a launch whose header does not say (n, C, H, W) runs no workgroup past its first lines
    const char *frag;
    const GrpRow *rows;
    uint8_t *y;              // [B][n][1][1]
    int out_cs, out_lead;
    int32_t *acc_out;
    float *y_f32;
    int zp_act, act, store_mode;
    float s_act;
    int32_t *ws_acc, *ws_sx; // S > 1: partial accumulators [S][B][npad] and partial sums of x' [S][B] (the caller's workspace)
    // geometry (set by the launcher)
    int mtiles, npad, fblocks;
    int S, sps;              // K slices and K-steps a slice
    int chunk, pitch;        // K-steps staged at a time; LDS bytes between two images (chunk bytes + 16)
};
int connected_launch(FcArgs &a, hipStream_t st);
// classify.hip: the global average pool, q = floor((2 S + HW) / (2 HW)) per image and channel
struct AvgArgs {
    const uint8_t *x;
    uint8_t *y;              // [B][C][1][1]
    int in_cs, in_lead, out_cs, out_lead;
    int B, H, W, C;
    int nchunks, dq, dr;     // set by the launcher: 64-byte channel chunks; 64 / W and 64 % W (a lane's step of 64 cells in rows and columns)
};
int avgpool_launch(AvgArgs &a, hipStream_t st);

// spp.hip: up to three stride-1 "same" max pools of one tensor in one launch (the SPP block of yolov3-spp / yolov4), computed as a
// cascade: level i is the box max of size d[i] of level i - 1, level 0 being x, so that level i is x's pool of size sizes[i].
constexpr int SPP_MAX = 3;       // levels
constexpr int SPP_RUN = 8;       // outputs along the pass direction per lane; also the smallest tile side
constexpr int SPP_TILE = 20;     // largest tile side: (20 + 12) rows of 33 cells of 32 bytes, twice, is 67 584 bytes of LDS
struct SppArgs {
    const uint8_t *x;            // input tensor, biased PHWC (cs % 16 == 0, data 16-byte aligned)
    int in_cs, in_lead;
    int B, H, W;
    int pieces16;                // 16-byte pieces of a cell that hold channels: ceil(C / 16); read and stored whole, as maxpool_u8_kernel does
    int n;                       // levels, 1..SPP_MAX
    int d[SPP_MAX];              // window of level i over level i - 1: sizes[i] - sizes[i - 1] + 1 (sizes[0] for level 0)
    uint8_t *y[SPP_MAX];         // each level's own tensor (x's B, H, W; data 16-byte aligned)
    int out_cs[SPP_MAX], out_lead[SPP_MAX];
    // tile geometry (set by the launcher)
    int R;                       // halo of the staged patch: (sizes[n - 1] - 1) / 2
    int TH, TW, tiles_x, tiles_y, nchunks;
    int ph, pw, pitch;           // staged patch: rows, cells per row, LDS cells between rows (odd)
    FastDiv fd_pw, fd_tw;
};
int spp_launch(SppArgs &a, hipStream_t st);

int yolo_detections_launch(const float *out, int B, int n, int classes, int h, int w, const float *biases, const int *mask,
                           int netw, int neth, int imw, int imh, float thresh, int relative, float *recs, int max_recs,
                           int *counts, hipStream_t st);
int conv_igemm_launch(ConvArgs &a, hipStream_t st);
int conv_rows_launch(ConvArgs &a, hipStream_t st, int bm, int bn);
int conv_small_pool_launch(ConvArgs &a, hipStream_t st);
// conv_small.hip's weights-stationary plane: A row R of a 32-filter m-tile holds filter ws_row_filter(R), so that the accumulator rows of
// one lane (8 grp + 4 kh + r in the 32 x 32 MFMA's D layout) are sixteen consecutive filters 16 kh + 4 grp + r
__host__ __device__ constexpr int ws_row_filter(int R) { return 16 * ((R >> 2) & 1) + 4 * (R >> 3) + (R & 3); }
bool conv_small_eligible(int n, int c, int ksize);
bool conv_pool16_eligible(int n, int c, int ksize);
int conv_pool16_launch(ConvArgs &a, hipStream_t st);  // conv_pool16.hip: c 16 | 32 + maxpool on 16 x 16 x 64 tiles (needs the blob's epilogue table)
bool conv_small32_eligible(int n, int c, int ksize);
int conv_small32_launch(ConvArgs &a, hipStream_t st);  // conv_small32.hip: c 32 -> n 64 + maxpool, eight waves per workgroup at four per SIMD (round 6)
int conv1x1_ws_launch(ConvArgs &a, hipStream_t st);
bool conv1x1_ws_eligible(int n, int c, int ksize);
int conv_ws3_launch(ConvArgs &a, hipStream_t st);
bool conv_ws3_eligible(int n, int c, int ksize);
int mi355_debug_flags_get();
// Every convolution launch site records its geometry just before hipLaunchKernelGGL (shim.hip: read back by mi355_last_conv_launch):
// workgroups, threads per workgroup, dynamic LDS bytes.  Host-side only, per calling thread.
void conv_launch_note(long grid, int threads, size_t lds);
// Throughput plan (mi355_conv_desc.plan): does this launch fit ONE round of whole-CU workgroups (128 x 384 output tiles, one
// per CU)?  Only such launches are re-planned into half-CU workgroups that share a CU with another batch's layer; a launch of
// several rounds keeps the whole-chip kernels, which are the more efficient ones and have their own tail to overlap
// (YOLOv3-608, batch 32: 128 -> 256 @76 83 -> 116 us, 256 -> 512 @38 84 -> 113 us when re-planned; profiles/r03_v3_plan_layers.log).
static inline bool plan_one_round(const ConvArgs &a)
{
    // ... and only maps that fill the row image of the 128-column kernel well (19-wide maps in 32-slot rows do not: YOLOv3's
    // 512 -> 1024 @19 layers 82 -> 100 us alone, 4.58 -> 4.64 ms per step with three batches in flight)
    const int rs = a.W + 2 <= 16 ? 16 : (a.W + 2 <= 32 ? 32 : 64);
    return a.plan == MI355_PLAN_THROUGHPUT && (long)((a.mpad + 127) / 128) * ((a.total_n + 383) / 384) <= 256 && 10 * (a.W + 2) >= 7 * rs;
}
int conv_first_launch(AuxArgs &a, hipStream_t st);
int conv_first_pool_launch(AuxArgs &a, hipStream_t st);
int conv_first_mfma_pool_launch(AuxArgs &a, hipStream_t st);
int conv_first_mfma_launch(AuxArgs &a, hipStream_t st);
int conv_ref_f32_launch(AuxArgs &a, hipStream_t st);
int maxpool_launch(const PoolArgs &a, hipStream_t st);
int copy_cells_launch(const CopyArgs &a, hipStream_t st);
int copy_cell_bytes_launch(const CopyArgs &a, int nbytes, hipStream_t st);
int nchw_to_phwc_launch(const LayoutArgs &a, hipStream_t st);
int phwc_to_nchw_launch(const LayoutArgs &a, hipStream_t st);
int dequant_cells_launch(const DequantArgs &a, hipStream_t st);
int shortcut_launch(const ShortcutArgs &a, hipStream_t st);
int fill_u32_launch(uint32_t *p, uint32_t v, long n, hipStream_t st);
int letterbox_launch(const float *im, int imw, int imh, int c, float *out, int w, int h, hipStream_t st);
int image_minmax_launch(const float *x, long count, uint32_t *mm, hipStream_t st);
int image_quantize_launch(const float *x, long count, float scale, int zp, uint8_t *out, hipStream_t st);
int image_minmax_batched_launch(const float *x, int B, long count, uint32_t *mm, hipStream_t st);
int image_quantize_per_image_launch(const float *x, int B, long count, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out,
                                    hipStream_t st);
int image_minmax_seed_launch(uint32_t *mm, int B, hipStream_t st);
// input_dev.hip: (scale, zero point) per image from the batch's min / max, and layer 0's bank entries from those pairs, on the device
int input_pairs_launch(const float *mm, int B, int shared, int32_t *entry, float *scale, uint8_t *zp, uint32_t *status, hipStream_t st);
int l0_derive_launch(const mi355_l0_consts *consts, int activation, void *bank, long entry_bytes, int B, int shared, float *scale, uint8_t *zp,
                     float *kept_scale, uint8_t *kept_zp, uint32_t *status, hipStream_t st);
// frames.hip: a kind of frames is a Source (Frame = its table entry in the C-ABI), instantiated there for these six
struct SourceU8;      // mi355_frame_u8
struct SourceYUV;     // mi355_frame_yuv
struct SourcePlanar;  // mi355_frame_planar
struct SourcePacked;  // mi355_frame_packed
struct SourceP010;    // mi355_frame_p010
struct SourceBayer;   // mi355_frame_bayer
template <class Source, class Frame> const char *frames_check(const Frame *host, int B, int w, int h);  // NULL, or why the batch is refused
template <class Source, class Frame> int frames_letterbox_minmax_launch(const Frame *table_dev, int B, int w, int h, uint32_t *mm, hipStream_t st);
template <class Source, class Frame>
int frames_letterbox_quantize_launch(const Frame *table_dev, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out,
                                     hipStream_t st);
// the same three for a batch whose slots look at their frames through views (one mi355_frame_view per slot)
template <class Source, class Frame>
const char *frames_view_check(const Frame *host, const mi355_frame_view *views_host, int B, int w, int h);
template <class Source, class Frame>
int frames_view_letterbox_minmax_launch(const Frame *table_dev, const mi355_frame_view *views_dev, int B, int w, int h, uint32_t *mm,
                                        hipStream_t st);
template <class Source, class Frame>
int frames_view_letterbox_quantize_launch(const Frame *table_dev, const mi355_frame_view *views_dev, int B, int w, int h,
                                          const float *scale_dev, const uint8_t *zp_dev, uint8_t *out, hipStream_t st);
// jpeg.hip: dequantise + inverse DCT of every block of a batch, then upsampling + colour into RGB frames.  The checks read the host
// mirror of the table and return NULL or why it is refused; the launchers take the grid from it.
const char *jpeg_idct_check(const mi355_jpeg_plane *host, int nplanes);
int jpeg_idct_launch(const mi355_jpeg_plane *table_dev, const mi355_jpeg_plane *table_host, int nplanes, hipStream_t st);
const char *jpeg_to_rgb_check(const mi355_jpeg_image *host, int B);
int jpeg_to_rgb_launch(const mi355_jpeg_image *table_dev, const mi355_jpeg_image *table_host, int B, hipStream_t st);
// png.hip: scanline reconstruction of every segment of a batch (one wave each), then de-interlacing + expansion into RGB frames
const char *png_unfilter_check(const mi355_png_segment *host, int nsegments);
int png_unfilter_launch(const mi355_png_segment *table_dev, int nsegments, hipStream_t st);
const char *png_to_rgb_check(const mi355_png_image *host, int B);
int png_to_rgb_launch(const mi355_png_image *table_dev, const mi355_png_image *table_host, int B, hipStream_t st);
// jpeg_entropy.hip: Huffman decoding of every segment of a batch, one workgroup each
const char *jpeg_entropy_check(const mi355_jpeg_segment *host, int nsegments, int subseq_bits);
int jpeg_entropy_launch(const mi355_jpeg_segment *table_dev, int nsegments, int subseq_bits, int *status_dev, hipStream_t st);
// png_inflate.hip: inflate of every deflate stream of a batch, one wave each
const char *png_inflate_check(const mi355_png_stream *host, int nstreams);
int png_inflate_launch(const mi355_png_stream *table_dev, int nstreams, int *status_dev, hipStream_t st);
int yolo_detections_sizes_launch(const float *out, int B, int n, int classes, int h, int w, const float *biases, const int *mask,
                                 int netw, int neth, const int *imw_dev, const int *imh_dev, float thresh, int relative, float *recs,
                                 int max_recs, int *counts, hipStream_t st);
int yolo_logistic_launch(const float *in, float *out, int B, int n, int classes, int hw, hipStream_t st);
// detect.hip: every head of a network, every image of the batch, records in reference order (mi355_yolo_detections_batch)
struct DetHead {
    const float *out, *biases;  // yolo output [B][n * (classes + 5)][h * w], anchors
    const int *mask;
    int n, h, w;
    int blk0;                   // first block (of 256 cells) of this head inside an image's row of blocks
};
struct DetBatchArgs {
    DetHead head[MI355_YOLO_MAX_HEADS];
    int nheads, B, classes, netw, neth, relative, max_per_image;
    int nblk;                   // blocks per image over all heads
    float thresh;
    const int *imw, *imh;       // [B], device
    float *recs;
    int *counts, *offsets;      // [B][nheads], [B + 1]
    int *work;                  // [B][nblk]: count of a block, then its exclusive offset inside the image
};
int yolo_detections_batch_launch(const DetBatchArgs &a, hipStream_t st);
int checksum_u32_launch(const uint32_t *p, long n, unsigned long long *out, hipStream_t st);

// Kernels with more than 64 KB of dynamic LDS need their limit raised: per kernel instantiation (the template argument) and per device --
// function attributes are per device, `darknet -gpus` drives several from one process -- and only when a launch needs more than the
// limit set so far, not once per launch.  (The limit counts against 160 KB TOGETHER with the kernel's static LDS: ask for what is needed.)
template <void (*kern)(const ConvArgs)>
static inline bool lds_limit_for(size_t lds)
{
    static size_t have[64] = {0};
    static std::mutex mu;  // host threads that drive replicas of one device may first-launch the same instantiation at the same time:
                           // the check, the attribute call and the record are one critical section (only taken when the limit has to grow)
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds <= 64 * 1024) return true;
    std::lock_guard<std::mutex> lk(mu);
    size_t &h = have[dev & 63];
    if (lds > h) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
        h = lds;
    }
    return true;
}
template <void (*kern)(const ConvArgs)>
static inline int launch_big_lds(int grid, int threads, size_t lds, hipStream_t st, const ConvArgs &a)
{
    if (!lds_limit_for<kern>(lds)) return MI355_EHIP;
    conv_launch_note(grid, threads, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
