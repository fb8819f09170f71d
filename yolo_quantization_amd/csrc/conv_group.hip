// conv_group.hip -- the grouped convolution (1 <= groups, c % groups == n % groups == 0) as a block-diagonal implicit
// GEMM on V_MFMA_I32_16X16X64_I8.
//
// Filter j belongs to group j / ng and reads the cg channels of that group only (cg = c / groups, ng = n / groups).  M = 16
// consecutive filters (tile t = filters 16 t ..), N = 16 output pixels, and a K-step is four SLOTS, one per 16-lane group of the wave:
// a slot is (piece, tap), a piece one 16-byte run of 16 input channels of a cell -- exactly a lane's B fragment.  The only property of
// the instruction relied on is that byte i of the A fragment of lane (m, q) meets byte i of the B fragment of lane (n, q).
//
// The block structure lives in the pack, not in the kernel.  The filters of a tile span some groups; their channels are one run of
// pieces, and the tile's K is the list of (piece, tap) slots over that run (kargs.h: cut into segments at group boundaries).  The A
// fragment of filter row r holds w' = w - 128 on the bytes of r's own group and 0 on every other byte: another group's channels in
// the piece, channels >= c, padding slots.  cg = ng = 16 is one piece per tile at full density, cg = 4 four groups per piece, cg = 12
// groups that straddle pieces, cg = 1 sixteen groups per piece, groups = 1 the dense layer: the kernel walks slot lists and sees none
// of these as cases.
//
// Zero points without a cross-lane step.  sum (w - zp_w) x = sum w'x' + d sum x' + [128 sum w' + 128 K d], d = 128 - zp_w, K = cg k k.
// sum x' runs over the row's own channels, so it differs from row to row: a second A fragment per K-step is 1 exactly where the row's
// weights are live, and its accumulator has the register layout of the one it corrects (lane l: rows 4 (l / 16) .. + 3 of pixel
// l % 16).  acc = acc1 + d[row] acc2 + cst[row], no shuffle; pad channels and pad slots mask themselves.
//
// Work split.  A workgroup (four waves) owns one image, a tile of 256 output pixels (64 when that does not fit) and a block of `mb`
// consecutive M tiles.  It stages only the pieces its block's filters read, once: each piece a plane of 16-byte cells over the
// ((TH - 1) s + k) x ((TW - 1) s + k) patch, bytes as they are in the tensor (x ^ 0x80), out-of-image cells zp_in ^ 0x80, so the MAC
// loop has no bounds check and the tensor's pad ring is never read.  Each wave takes 16 NT pixels and walks the block's tiles one
// after another: per K-step NT B fragments from LDS, the weight and indicator fragments and the slot entry from global memory one
// step ahead, 2 NT MFMAs; then the tile's epilogue (common.h requant_u8, or requant_q_exact when every shift is a power of two).
// When not even one tile's pieces fit beside each other, the segments of a tile are staged one after another (`restage`).
#include "kargs.h"
#include <mutex>

namespace {

constexpr int GRP_THREADS = 256;
constexpr size_t GRP_LDS_MAX = 160 * 1024;

__device__ __forceinline__ uint32_t grp_finish(int32_t q, int zp_act, int act, int store_mode)
{
    // requant_u8's second half (common.h): activation, zero point, store mode, uint8 wrap
    int32_t v;
    if (act == MI355_ACT_LEAKY) {
        const uint32_t uq = 0u - (uint32_t)q;
        v = q < 0 ? zp_act - (int32_t)((uq + 5u) / 10u) : q + zp_act;
    } else if (act == MI355_ACT_RELU6) {
        v = q <= 0 ? zp_act : q + zp_act;
    } else {
        v = q + zp_act;
    }
    if (store_mode == MI355_STORE_SATURATE) v = v < 0 ? 0 : (v > 255 ? 255 : v);
    return (uint32_t)v & 0xFFu;
}

// NT: 16-pixel N tiles per wave (4: 256 pixels per workgroup, 1: 64); RESTAGE: a segment's pieces are staged when it is walked
template <int NT, bool RESTAGE>
__global__ __launch_bounds__(GRP_THREADS) void conv_group_kernel(const GrpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *tapoff = reinterpret_cast<int *>(smem);  // [GRP_MAX_TAPS] cell offset of tap t from a pixel's window origin
    char *P = smem + GRP_MAX_TAPS * sizeof(int);  // [piece][plane] cells of 16 bytes

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lp = lane & 15, q = lane >> 4;
    const int k = a.ksize, kk = k * k, s = a.stride, pw = a.pw, ncells = a.ph * a.pw, plane = a.plane;
    const int TW = 1 << a.tw_sh, TH = (64 * NT) >> a.tw_sh;

    const int fb = blockIdx.x % a.fblocks;
    int nt = blockIdx.x / a.fblocks;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = nt / tpi;
    nt -= b * tpi;
    const int tyi = nt / a.tiles_x, txi = nt - tyi * a.tiles_x;
    const int oy0 = tyi * TH, ox0 = txi * TW;
    const int iy0 = oy0 * s - a.pad, ix0 = ox0 * s - a.pad;

    for (int t = tid; t < GRP_MAX_TAPS; t += GRP_THREADS) tapoff[t] = t < kk ? (t / k) * pw + (t % k) : 0;

    int cbase[NT];  // window origin (patch cell of tap (0, 0)) of this lane's pixels
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int p = (wave * NT + j) * 16 + lp;
        cbase[j] = (p >> a.tw_sh) * s * pw + (p & (TW - 1)) * s;
    }
    const int W1 = a.W + 1, OW1 = a.OW + 1, ohw = a.OH * a.OW;
    const uint32_t fill = (uint32_t)((a.zp_in ^ 0x80) & 0xFF) * 0x01010101u;

    // pieces [pf, pf + np) of the patch into planes 0 .. np - 1: in-image cells from the tensor, the rest the biased input zero point
    auto stage = [&](int pf, int np) {
        for (int i = tid; i < np * ncells; i += GRP_THREADS) {
            const int u = i / ncells, cell = i - u * ncells;
            const int r = cell / pw, cc = cell - r * pw;
            const int iy = iy0 + r, ix = ix0 + cc;
            uint4 v = make_uint4(fill, fill, fill, fill);
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v = *reinterpret_cast<const uint4 *>(a.x + (size_t)((long)a.in_lead + ((long)b * (a.H + 1) + iy + 1) * W1 + ix) * a.in_cs +
                                                     (size_t)(pf + u) * 16);
            *reinterpret_cast<uint4 *>(P + ((size_t)u * plane + cell) * 16) = v;
        }
    };

    const int t0 = fb * a.mb, t1 = min(t0 + a.mb, a.mtiles);
    const int s0 = a.tseg[t0], s1 = a.tseg[t1];
    const int P0 = a.seg[s0].p0;
    if constexpr (!RESTAGE) stage(P0, a.seg[s1 - 1].p0 + a.seg[s1 - 1].npieces - P0);
    __syncthreads();
    const bool pow2 = a.hdr->pow2 == 1;

    v4i acc1[NT] = {}, acc2[NT] = {};
#pragma unroll 1
    for (int sg = s0; sg < s1; ++sg) {
        const GrpSeg g = a.seg[sg];
        if constexpr (RESTAGE) {
            __syncthreads();  // the previous segment's cells are read
            stage(g.p0, g.npieces);
            __syncthreads();
        }
        const int pl0 = RESTAGE ? 0 : (g.p0 - P0) * plane;
        if (g.first) {
#pragma unroll
            for (int j = 0; j < NT; ++j) acc1[j] = acc2[j] = v4i{0, 0, 0, 0};
        }
        // slot entry of this lane's 16-lane group and the two A fragments, read one K-step ahead
        const int *slots = reinterpret_cast<const int *>(a.frag + (size_t)g.off16 * 16) + q;
        const v4i *fr = reinterpret_cast<const v4i *>(a.frag + (size_t)g.off16 * 16 + (size_t)g.nsteps * 16) + lane;
        int sn = slots[0];
        v4i wn = fr[0], in = fr[64];
#pragma unroll 1
        for (int st = 0; st < g.nsteps; ++st) {
            const int sc = sn;
            const v4i wf = wn, jf = in;
            if (st + 1 < g.nsteps) {
                sn = slots[4 * (st + 1)];
                wn = fr[(size_t)(st + 1) * 128];
                in = fr[(size_t)(st + 1) * 128 + 64];
            }
            const int off = pl0 + (sc >> 8) * plane + tapoff[sc & 0xFF];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const v4i bf = *reinterpret_cast<const v4i *>(P + (size_t)(cbase[j] + off) * 16);
                acc1[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, bf, acc1[j], 0, 0, 0);
                acc2[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(jf, bf, acc2[j], 0, 0, 0);
            }
        }
        if (!g.last) continue;

        // ---- epilogue of the tile: lane (lp, q) holds pixel lp and filter rows 4 q .. 4 q + 3 of both accumulators
        const int row0 = g.tile * 16 + 4 * q;
        if (row0 >= a.n) continue;
        GrpRow rw[4];  // (the per-filter records are padded to whole tiles)
#pragma unroll
        for (int r = 0; r < 4; ++r) rw[r] = a.rows[row0 + r];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int p = (wave * NT + j) * 16 + lp;
            const int oy = oy0 + (p >> a.tw_sh), ox = ox0 + (p & (TW - 1));
            if (oy >= a.OH || ox >= a.OW) continue;
            const size_t pix = (size_t)oy * a.OW + ox;
            uint32_t bytes[4] = {0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int oc = row0 + r;
                if (oc >= a.n) break;
                const uint32_t acct = (uint32_t)acc1[j][r] + (uint32_t)rw[r].d * (uint32_t)acc2[j][r] + (uint32_t)rw[r].cst;
                uint32_t u8;
                if (pow2) u8 = grp_finish(requant_q_exact((int32_t)(acct + (uint32_t)rw[r].bias), rw[r].mprime), a.zp_act, a.act, a.store_mode);
                else u8 = requant_u8((int32_t)acct, rw[r].bias, rw[r].mval, rw[r].sval, a.zp_act, a.act, a.store_mode);
                bytes[r] = u8;
                const size_t ridx = ((size_t)b * a.n + oc) * ohw + pix;
                if (a.acc_out) a.acc_out[ridx] = (int32_t)acct;
                if (a.y_f32) a.y_f32[ridx] = (float)((int)u8 - a.zp_act) * a.s_act;
            }
            if (a.y) {
                uint8_t *dst = a.y + (size_t)((long)a.out_lead + ((long)b * (a.OH + 1) + oy + 1) * OW1 + ox) * a.out_cs + row0;
                if (row0 + 3 < a.n) {
                    *reinterpret_cast<uint32_t *>(dst) = (bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24) ^ 0x80808080u;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row0 + r < a.n) dst[r] = (uint8_t)(bytes[r] ^ 0x80u);
                }
            }
        }
    }
}

// dynamic LDS above the 64 KiB default: raised per instantiation and device, only when a launch needs more (kargs.h lds_limit_for)
template <void (*kern)(const GrpArgs)>
int grp_launch_one(const GrpArgs &a, int grid, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        static size_t have[64] = {0};
        static std::mutex mu;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(mu);
        size_t &h = have[dev & 63];
        if (lds > h) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return MI355_EHIP;
            h = lds;
        }
    }
    conv_launch_note(grid, GRP_THREADS, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(GRP_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

// most pieces any block of mb consecutive M tiles reads (mb == 0: most pieces of any one segment)
int grp_max_pieces(const GrpArgs &a, int mb)
{
    const int cg = a.c / a.groups, ng = a.n / a.groups;
    int most = 0;
    if (mb == 0) {
        int p0[16], np[16], qa[16], qb[16];
        for (int t = 0; t < a.mtiles; ++t)
            for (int i = grp_tile_segs(a.n, a.c, a.groups, t, p0, np, qa, qb); i-- > 0;) most = np[i] > most ? np[i] : most;
        return most;
    }
    for (int t0 = 0; t0 < a.mtiles; t0 += mb) {
        const int t1 = t0 + mb < a.mtiles ? t0 + mb : a.mtiles;
        const int ga = 16 * t0 / ng, jl = 16 * t1 - 1 < a.n ? 16 * t1 - 1 : a.n - 1;
        const int np = (int)(((long)(jl / ng + 1) * cg - 1) / 16) - (int)((long)ga * cg / 16) + 1;
        most = np > most ? np : most;
    }
    return most;
}

}  // namespace

int conv_group_launch(GrpArgs &a, hipStream_t st)
{
    if (!grp_domain(a.n, a.c, a.groups, a.ksize) || a.stride < 1 || a.pad < 0 || a.OH < 1 || a.OW < 1) return MI355_EINVAL;
    if (a.in_cs % 16 || a.in_cs < (a.c + 15) / 16 * 16 || ((uintptr_t)a.x & 15) || ((uintptr_t)a.frag & 15)) return MI355_EINVAL;
    a.mtiles = (a.n + 15) / 16;
    // 256 pixels (32 x 8, 16 x 16 or 8 x 32 by the output width) with the largest block of M tiles whose pieces fit in LDS, the
    // throughput plan first within half of it (two workgroups per CU); then 64 pixels (8 x 8, 4 x 16, 2 x 32) the same way; then 64
    // pixels and one M tile whose segments are staged one after another
    const int tw = a.OW <= 8 ? 8 : (a.OW <= 16 ? 16 : 32);
    a.tw_sh = tw == 8 ? 3 : (tw == 16 ? 4 : 5);
    for (int npx : {256, 64}) {
        const int th = npx / tw;
        const long ph = (long)(th - 1) * a.stride + a.ksize, pw = (long)(tw - 1) * a.stride + a.ksize;
        if (ph * pw > (long)(GRP_LDS_MAX / 16)) continue;
        a.ph = (int)ph; a.pw = (int)pw; a.plane = (int)(ph * pw) | 1;
        a.tiles_x = (a.OW + tw - 1) / tw; a.tiles_y = (a.OH + th - 1) / th;
        auto lds_of = [&](int pieces) { return GRP_MAX_TAPS * sizeof(int) + (size_t)pieces * a.plane * 16; };
        int mb = 0, pieces = 0;
        for (size_t cap : {a.plan == MI355_PLAN_THROUGHPUT ? GRP_LDS_MAX / 2 : GRP_LDS_MAX, GRP_LDS_MAX}) {
            for (int cand : {8, 4, 2, 1}) {
                pieces = grp_max_pieces(a, cand);
                if (lds_of(pieces) <= cap) { mb = cand; break; }
            }
            if (mb) break;
        }
        a.restage = 0;
        if (!mb && npx == 64) {
            pieces = grp_max_pieces(a, 0);
            if (lds_of(pieces) > GRP_LDS_MAX) return MI355_EINVAL;
            mb = 1; a.restage = 1;
        }
        if (!mb) continue;
        a.mb = mb; a.fblocks = (a.mtiles + mb - 1) / mb;
        const long grid = (long)a.fblocks * a.B * a.tiles_x * a.tiles_y;
        if (grid > 0x7FFFFFFF) return MI355_EINVAL;
        if (npx == 256) return grp_launch_one<conv_group_kernel<4, false>>(a, (int)grid, lds_of(pieces), st);
        if (!a.restage) return grp_launch_one<conv_group_kernel<1, false>>(a, (int)grid, lds_of(pieces), st);
        return grp_launch_one<conv_group_kernel<1, true>>(a, (int)grid, lds_of(pieces), st);
    }
    return MI355_EINVAL;
}
