// input_dev.hip -- the input scales and layer 0's constants derived on the device (mi355_input_pairs, mi355_l0_derive).
//
// Only layer 0 depends on the input (scale, zero point).  The host path copies every batch's min / max down, waits, evaluates the
// reference's expressions, re-derives layer 0 (prep_conv_layer + mi355_conv_pack + mi355_conv_pack_epilogue) and uploads it.  The two
// kernels below do the same arithmetic where the min / max already are: image_scale_zero_point (network.c; ref: src/blas.c:125-150), then
// the parameter half of the prep (ref: src/blas.c:300-333, :387-418) and everything ept_fill (shim.hip) writes, into a bank slot that
// was initialised with a packed layer-0 blob -- so the weights and everything else that does not depend on the pair are in place already.
// Every byte equals the host prep's: the same C expressions in the same types, -ffp-contract=off, IEEE division, and the epilogue
// table through the functions the host calls (common.h: small_safe_range, biased_safe_range, intrq_make, leaky_byte_biased, ept_key).
#include "kargs.h"

// ---------------------------------------------------------------------------------------------------------------
// (scale, zero point) of image b from mm[2 b] = max, mm[2 b + 1] = min as the min / max kernels leave them (glue.hip, frames.hip).
// shared: image 0's pair in every slot.  Where the host dies (an all-zero image, a zero scale) the slot keeps the pair it held.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void input_pairs_kernel(const float *mm, int B, int shared, int32_t *entry, float *scale, uint8_t *zp,
                                                          uint32_t *status)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int src = shared ? 0 : b;
    const float max_value = mm[2 * src], min_value = mm[2 * src + 1] + 0.0f;  // (+ 0.0f: the call sites' canonical zero)
    uint32_t st = 0;
    if (min_value == 0 && max_value == 0) {
        st = MI355_INPUT_ALL_ZERO;
    } else {
        const float nudged_scale = (max_value - min_value) * (1.0f / 255.0f);
        if (nudged_scale == 0) {
            st = MI355_INPUT_ZERO_SCALE;
        } else {
            const double initial_zero_point = (double)(0.0f - min_value / nudged_scale);
            uint8_t z;
            if (initial_zero_point < 0) z = 0;
            else if (initial_zero_point > 255) z = 255;
            else z = (uint8_t)round(initial_zero_point);
            scale[b] = nudged_scale;
            zp[b] = z;
        }
    }
    status[b] = st;
    if (entry) entry[b] = shared ? 0 : b;
}

int input_pairs_launch(const float *mm, int B, int shared, int32_t *entry, float *scale, uint8_t *zp, uint32_t *status, hipStream_t st)
{
    hipLaunchKernelGGL(input_pairs_kernel, dim3((B + 255) / 256), dim3(256), 0, st, mm, B, shared, entry, scale, zp, status);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

// ---------------------------------------------------------------------------------------------------------------
// One channel of prep_conv_layer (network.c) for input scale s_in / zero point zp_in, with mi355_conv_pack's range checks.
// ---------------------------------------------------------------------------------------------------------------
struct L0Chan {
    uint32_t fail;    // MI355_INPUT_* bits: where the host prep dies or mi355_conv_pack refuses
    int32_t shift, bias;
    double mval, sval;
};

__device__ static L0Chan l0_channel(const mi355_l0_consts &c, const mi355_l0_channel &ch, float s_in, int zp_in)
{
    L0Chan r;
    r.fail = 0; r.shift = 0; r.bias = 0; r.mval = 0; r.sval = 0;
    const uint32_t mult_zero_point = (uint32_t)(c.K * zp_in * ch.w_zp);
    const int32_t weights_sum_int = (int32_t)(mult_zero_point - (uint32_t)(ch.wsum * zp_in));
    float real_multiplier = s_in * ch.w_scale / c.s_act;
    if (!(real_multiplier > 0.f) || !(real_multiplier < 1.f)) { r.fail = MI355_INPUT_M_RANGE; return r; }
    int s = 0;
    while (real_multiplier < 0.5f) {
        real_multiplier *= 2.0f;
        s++;
    }
    int64_t q = (int64_t)round((double)(real_multiplier * (float)(1ll << 31)));
    if (q == (1ll << 31)) {
        q /= 2;
        s--;
    }
    if (s < 0) { r.fail = MI355_INPUT_NEG_SHIFT; return r; }
    r.shift = s;
    r.sval = __longlong_as_double((long long)(1023 - s) << 52);   // pow(2, -s): s <= 149 for a positive float M
    r.mval = 4.656612873077392578125e-10 * (double)(int32_t)q;     // pow(2, -31) * M0
    if (!(r.mval > 0.0 && r.mval < 1.0) || !(r.sval > 0.0 && r.sval <= 1.0)) { r.fail = MI355_INPUT_PACK_RANGE; return r; }
    const float t = ch.bias / (s_in * ch.w_scale) + (float)weights_sum_int;
    if (!(t >= -2147483648.0f && t < 2147483648.0f)) { r.fail = MI355_INPUT_BIAS_RANGE; return r; }
    r.bias = (int32_t)t;
    return r;
}

// Is the slot a first-layer blob of this shape with every section inside the slot?  (The kernel takes the section offsets from the
// slot's own header: nothing is written through them before this holds.)
__device__ static bool l0_slot_ok(const ConvBlobHeader &h, int n, long entry_bytes)
{
    if (h.magic != MI355_BLOB_MAGIC || h.n != n || h.c != 3 || h.ksize != 3 || !h.first || h.mpad < n || h.mpad > n + 3) return false;
    if ((long)h.total > entry_bytes || !h.off_ept) return false;
    const uint64_t m = (uint64_t)h.mpad, t = h.total;
    const uint64_t ept = sizeof(EptHeader) + m * sizeof(EptEntry) + (uint64_t)LUTQ_N + (uint64_t)((n + 15) / 16) * 64 * sizeof(L0Lane);
    return h.off_cw + 4 * m <= t && h.off_dzp + 4 * m <= t && h.off_bias + 4 * m <= t && h.off_mval + 8 * m <= t && h.off_sval + 8 * m <= t &&
           h.off_shift + 4 * m <= t && h.off_mprime + 8 * m <= t && h.off_cwb + 4 * m <= t && h.off_ept + ept <= t;
}

// One workgroup per entry.  Entry e is derived from image e's pair; shared: one entry, image 0's pair, and what is written per image
// (status, the kept pair) goes to every image.  Three passes over the channels with a workgroup-wide reduction after each: (1) does any
// channel fail, is every shift <= 31 (the header's pow2); (2) the per-channel parameters and table entries, OR of the EPT_* flags;
// (3) what depends on those flags (the byte table) or on other threads' entries (the lane records).  Nothing is written before (1) passed.
template <int ACT>
__global__ __launch_bounds__(256) void l0_derive_kernel(const mi355_l0_consts *consts, char *bank, long entry_bytes, int B, int shared,
                                                        float *scale, uint8_t *zp, float *kept_scale, uint8_t *kept_zp, uint32_t *status)
{
    __shared__ uint32_t sh_fail, sh_not_pow2, sh_flags;
    const int tid = threadIdx.x, e = blockIdx.x;
    char *base = bank + (long)e * entry_bytes;
    const ConvBlobHeader h = *reinterpret_cast<const ConvBlobHeader *>(base);
    const mi355_l0_consts c = *consts;
    const mi355_l0_channel *chans = reinterpret_cast<const mi355_l0_channel *>(consts + 1);
    const int n = c.n;
    const float s_in = scale[e];
    const int zp_in = zp[e];
    const int b0 = shared ? 0 : e, b1 = shared ? B : e + 1;   // the images this entry serves
    if (tid == 0) { sh_fail = l0_slot_ok(h, n, entry_bytes) ? 0u : MI355_INPUT_BAD_SLOT; sh_not_pow2 = 0; sh_flags = 0; }
    __syncthreads();
    {
        uint32_t fail = 0, np2 = 0;
        for (int oc = tid; oc < n; oc += blockDim.x) {
            const L0Chan r = l0_channel(c, chans[oc], s_in, zp_in);
            fail |= r.fail;
            np2 |= (uint32_t)(r.shift > 31);
        }
        if (fail) atomicOr(&sh_fail, fail);
        if (np2) atomicOr(&sh_not_pow2, 1u);
    }
    __syncthreads();
    if (sh_fail) {  // the slot stays the valid entry it was, its images keep the pair it was derived from
        for (int b = b0 + tid; b < b1; b += blockDim.x) {
            status[b] |= sh_fail;
            scale[b] = kept_scale[b];
            zp[b] = kept_zp[b];
        }
        return;
    }
    const bool pow2 = !sh_not_pow2;
    int32_t *bias = reinterpret_cast<int32_t *>(base + h.off_bias), *shift = reinterpret_cast<int32_t *>(base + h.off_shift);
    int32_t *cwb = reinterpret_cast<int32_t *>(base + h.off_cwb);
    const int32_t *cw = reinterpret_cast<const int32_t *>(base + h.off_cw), *dzp = reinterpret_cast<const int32_t *>(base + h.off_dzp);
    double *mval = reinterpret_cast<double *>(base + h.off_mval), *sval = reinterpret_cast<double *>(base + h.off_sval);
    double *mprime = reinterpret_cast<double *>(base + h.off_mprime);
    EptHeader *eh = reinterpret_cast<EptHeader *>(base + h.off_ept);
    EptEntry *ent = reinterpret_cast<EptEntry *>(eh + 1);
    {
        uint32_t flags = pow2 ? EPT_POW2 : EPT_NOINT;
        for (int oc = tid; oc < n; oc += blockDim.x) {
            const L0Chan r = l0_channel(c, chans[oc], s_in, zp_in);
            const int32_t cwb_oc = (int32_t)((uint32_t)cw[oc] + (uint32_t)r.bias);
            const double mp = r.mval * r.sval;
            bias[oc] = r.bias; mval[oc] = r.mval; sval[oc] = r.sval;
            shift[oc] = pow2 ? r.shift : 0;
            cwb[oc] = cwb_oc;
            mprime[oc] = mp;
            int32_t lo, hi, lb = 0, m0 = 0, sh = 0;
            uint32_t rg = 0;
            small_safe_range<ACT>(mp, c.zp_act, lo, hi);
            if (!biased_safe_range(lo, hi, lb, rg)) flags |= EPT_NEVER;
            if (!pow2 || !intrq_make(r.mval, r.shift, lb, (int32_t)((uint32_t)lb + rg), m0, sh, ACT == MI355_ACT_RELU6)) {
                flags |= EPT_NOINT;
                m0 = sh = 0;
            }
            EptEntry t;
            t.lb = lb; t.rg = rg; t.m0 = m0; t.sh = sh;
            t.qc = (int64_t)lb * (int64_t)m0;
            t.cbl = (int32_t)((uint32_t)cwb_oc - (uint32_t)lb);
            t.pad_ = 0;
            ent[oc] = t;
            if (dzp[oc] > 127) flags |= EPT_D2;
        }
        atomicOr(&sh_flags, flags);
    }
    __syncthreads();  // the entries of every channel are written, the flags complete
    const uint32_t flags = sh_flags;
    uint8_t *lut = reinterpret_cast<uint8_t *>(ent + h.mpad);
    {
        const bool by_floor = !(flags & EPT_NOINT);
        for (int i = tid; i < LUTQ_N / 4; i += blockDim.x) {
            uint32_t w = 0;
            if (ACT == MI355_ACT_LEAKY) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int f = 4 * i + k - LUTQ_OFF;
                    w |= (leaky_byte_biased<false>(by_floor && f < 0 ? f + 1 : f, c.zp_act) & 0xFFu) << (8 * k);
                }
            }
            reinterpret_cast<uint32_t *>(lut)[i] = w;
        }
    }
    L0Lane *ll = reinterpret_cast<L0Lane *>(lut + LUTQ_N);
    for (int idx = tid; idx < ((n + 15) / 16) * 64; idx += blockDim.x) {
        const int mt = idx >> 6, g = (idx & 63) >> 4;
        L0Lane &L = ll[idx];
        for (int r = 0; r < 4; ++r) {
            const int c2 = 16 * mt + 4 * g + r;
            if (c2 >= n) continue;
            const EptEntry t = ent[c2];
            L.cb[r] = t.cbl; L.lo[r] = t.lb; L.hi[r] = (int32_t)t.rg;
            L.qm0[r] = t.m0; L.qsh[r] = t.sh; L.qc[r] = t.qc;
            L.mp[r] = mprime[c2];
        }
    }
    if (tid == 0) {
        reinterpret_cast<ConvBlobHeader *>(base)->pow2 = pow2 ? 1 : 0;
        eh->flags = flags;
        eh->pad_[0] = eh->pad_[1] = 0;
        eh->key = ept_key(ACT, c.zp_act);
    }
    for (int b = b0 + tid; b < b1; b += blockDim.x) {  // the pair this entry now stands for
        kept_scale[b] = s_in;
        kept_zp[b] = (uint8_t)zp_in;
    }
}

int l0_derive_launch(const mi355_l0_consts *consts, int activation, void *bank, long entry_bytes, int B, int shared, float *scale, uint8_t *zp,
                     float *kept_scale, uint8_t *kept_zp, uint32_t *status, hipStream_t st)
{
    const dim3 grid(shared ? 1 : B), block(256);
    char *bk = (char *)bank;
    switch (activation) {
    case MI355_ACT_LEAKY:
        hipLaunchKernelGGL(l0_derive_kernel<MI355_ACT_LEAKY>, grid, block, 0, st, consts, bk, entry_bytes, B, shared, scale, zp, kept_scale, kept_zp, status);
        break;
    case MI355_ACT_RELU6:
        hipLaunchKernelGGL(l0_derive_kernel<MI355_ACT_RELU6>, grid, block, 0, st, consts, bk, entry_bytes, B, shared, scale, zp, kept_scale, kept_zp, status);
        break;
    case MI355_ACT_RELU:  // as mi355_conv_pack_epilogue: the LINEAR table serves both
    case MI355_ACT_LINEAR:
        hipLaunchKernelGGL(l0_derive_kernel<MI355_ACT_LINEAR>, grid, block, 0, st, consts, bk, entry_bytes, B, shared, scale, zp, kept_scale, kept_zp, status);
        break;
    default: return MI355_EINVAL;
    }
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
