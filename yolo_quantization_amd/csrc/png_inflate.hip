// png_inflate.hip -- mi355_png_inflate: inflate (RFC 1951) of the IDAT streams of a batch on the device, the step in front of png.hip.
// One 64-thread workgroup -- one wave -- per stream.  Deflate has no block index, so the symbols of a stream are followed by one lane,
// lane 0, through host/png_inflate_core.h (the text the host emulation runs); everything else is done by all lanes.  In LDS (71 KB):
// the 64 KiB ring of the output, the literal/length and the distance table of the current block (a 10-bit look table plus the
// count[] / symbol[] walk for longer codes), the code lengths, a 1 KiB window of the input and the token list.  The wave works in steps,
// each a step of the stream's state machine (pic_state.phase):
//   window   all lanes load the next 256 dwords of the stream into LDS; lane 0's bit reader refills from there;
//   header   lane 0 reads a block header: LEN / NLEN of a stored block, or the code lengths (fixed, or HLIT / HDIST / HCLEN and the
//            repeat codes), the over-subscription check and the codes of every symbol; then all lanes zero and fill both look tables;
//   round    lane 0 decodes up to 64 tokens (a literal, or length << 16 | distance) -- the round ends at 64, at the end of the block, at
//            cap or at an error --; a wave scan of the tokens' lengths gives lane t the output position of token t; all lanes place the
//            literals; the matches go in token order, all lanes copying one match with src[j % dist], which reads only bytes in front of
//            the match (final: earlier tokens) and so has no dependence inside an overlapping copy;
//   stored   all lanes copy up to 16 KiB of a stored block from the stream into the ring;
//   flush    once 16 KiB are waiting (and at the end) all lanes store the ring's finished bytes to `out`, a dword a lane.
// The ring is 64 KiB, not 32: a round produces up to 64 * 258 bytes, and the literals of a round are placed before its matches, so a
// ring of exactly the window would let a late literal overwrite a byte an earlier match of the round still reads at distance 32767.
// With 64 KiB every byte a round reads (>= its start - 32768) and writes (< its start + 16512) has a slot of its own.
// The tables and the window are written by this wave and read through LDS, never through scalar loads.
//
// Bounds.  Every step consumes at least one bit of the stream, or produces at least one byte, or ends the stream; consuming a bit
// past the end is an error (bits past the end read as zero), and cap ends the decode: at most 8 * nbytes + 64 symbol steps and cap
// output bytes.  No wave waits for another.  Reads of the stream stay inside z[0, round4(nbytes) + 8): the window load clamps word
// indices and the stored copy is checked against nbytes before it starts.  Writes go to out[0, cap) -- n never passes cap: a match is
// cut at it -- and to the stream's status word.  A distance above the bytes produced is MI355_PNG_EDIST, never an address; no table is
// used after a failed build; a symbol no code has is MI355_PNG_EHUFF.
#include "kargs.h"
#include "../host/png_inflate_core.h"

constexpr int PNGI_LANES = 64;

__global__ __launch_bounds__(PNGI_LANES) void png_inflate_kernel(const mi355_png_stream *table, int *status)
{
    __shared__ uint8_t ring[PIC_RING];
    __shared__ pic_code zl, zd;
    __shared__ uint32_t window[PIC_WINDOW];
    __shared__ uint32_t tok[PIC_TOKENS], tok_at[PIC_TOKENS];
    __shared__ uint16_t codes[PIC_MAX_LENS];
    __shared__ uint8_t lens[PIC_MAX_LENS];
    __shared__ pic_state st;
    const int lane = threadIdx.x;
    const mi355_png_stream &t = table[blockIdx.x];
    const uint32_t *z = t.z;
    uint8_t *out = t.out;
    const uint32_t nbytes = t.nbytes, cap = t.cap, nwords = pic_stream_words(nbytes);
    constexpr uint32_t M = PIC_RING - 1;

    if (lane == 0) {
        pic_state s = {};
        s.b.w = window; s.b.nw = PIC_WINDOW; s.b.nbytes = nbytes;
        s.cap = cap;
        st = s;
    }
    uint32_t flushed = 0;  // the same in every lane
    __syncthreads();

    for (;;) {
        const int phase = st.phase;
        if (phase == PIC_DONE) break;
        if (phase != PIC_STORED) {
            // window: words next .. next + 255 of the stream, zero where the stream's readable words end
            const uint32_t base = st.b.next;
            for (int k = lane; k < PIC_WINDOW; k += PNGI_LANES) {
                const uint32_t wi = base + (uint32_t)k;
                window[k] = wi < nwords ? z[wi] : 0u;
            }
            if (lane == 0) st.b.base = base;
            __syncthreads();
        }
        if (phase == PIC_HEADER) {
            if (lane == 0) pic_header(&st, &zl, &zd, lens, codes);
            __syncthreads();
            if (st.phase == PIC_BUILD) {
                const int hlit = st.hlit, hdist = st.hdist;
                pic_look_zero(&zl, lane, PNGI_LANES);
                pic_look_zero(&zd, lane, PNGI_LANES);
                __syncthreads();
                pic_look_fill(&zl, lens, hlit, codes, lane, PNGI_LANES);
                pic_look_fill(&zd, lens + hlit, hdist, codes + hlit, lane, PNGI_LANES);
                if (lane == 0) st.phase = PIC_SYMBOLS;
            }
        } else if (phase == PIC_SYMBOLS) {
            if (lane == 0) pic_round(&st, &zl, &zd, tok, window);
            __syncthreads();
            const int ntok = st.ntok;
            // the scan: token `lane`'s first output byte
            const uint32_t mine = lane < ntok ? tok[lane] : 0u;
            const uint32_t mylen = lane < ntok ? (mine >> 16 ? mine >> 16 : 1u) : 0u;
            uint32_t incl = mylen;
            for (int d = 1; d < PNGI_LANES; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            const uint32_t at = st.n0 + incl - mylen;
            tok_at[lane] = at;
            if (lane < ntok && !(mine >> 16)) ring[at & M] = (uint8_t)mine;
            __syncthreads();
            for (int k = 0; k < ntok; ++k) {
                const uint32_t m = tok[k], len = m >> 16, dist = m & 0xffffu;
                if (!len) continue;  // (uniform: every lane reads the same token)
                const uint32_t p = tok_at[k], from = p - dist;
                if (dist >= len) {
                    for (uint32_t j = lane; j < len; j += PNGI_LANES) ring[(p + j) & M] = ring[(from + j) & M];
                } else {
                    for (uint32_t j = lane; j < len; j += PNGI_LANES) ring[(p + j) & M] = ring[(from + j % dist) & M];
                }
                __syncthreads();  // the next match may read these bytes
            }
        } else {  // PIC_STORED
            const uint32_t left = st.stored_left, chunk = left < PIC_STORED_CHUNK ? left : PIC_STORED_CHUNK, n = st.n;
            const uint8_t *src = reinterpret_cast<const uint8_t *>(z) + st.stored_at;  // [stored_at, stored_at + left) lies inside nbytes
            for (uint32_t j = lane; j < chunk; j += PNGI_LANES) ring[(n + j) & M] = src[j];
            __syncthreads();  // every lane has read the state
            if (lane == 0) pic_stored_done(&st, chunk);
        }
        __syncthreads();
        // flush: [flushed, to) of the ring, dwords; flushed stays a multiple of 4 and out is 4-byte aligned
        const uint32_t n = st.n;
        const bool done = st.phase == PIC_DONE;
        if (n - flushed >= PIC_STORED_CHUNK || done) {
            const uint32_t to = n & ~3u;
            for (uint32_t i = flushed + 4u * (uint32_t)lane; i < to; i += 4u * PNGI_LANES)
                *reinterpret_cast<uint32_t *>(out + i) = *reinterpret_cast<const uint32_t *>(&ring[i & M]);
            if (done && to + (uint32_t)lane < n) out[to + lane] = ring[(to + lane) & M];
            flushed = to;
        }
        __syncthreads();  // the ring, the window and the tokens are rewritten by the next step
    }

    // the status, in the host decoder's order: the stream's, then the length, then the filter bytes
    int code = st.status;
    if (!code && st.n < cap) code = MI355_PNG_EPIXELS;
    if (!code) {
        __threadfence();  // this wave's stores to out, read back below
        int bad = 0;
        const volatile uint8_t *row = out;
        for (int k = 0; k < t.npasses; ++k) {
            const uint32_t rows = (uint32_t)t.rows[k], pitch = (uint32_t)t.row_bytes[k] + 1u;
            for (uint32_t y = lane; y < rows; y += PNGI_LANES) bad |= row[(size_t)y * pitch] > 4;
            row += (size_t)rows * pitch;
        }
        if (__any(bad)) code = MI355_PNG_EFILTER;
    }
    if (lane == 0) status[blockIdx.x] = code;
}

const char *png_inflate_check(const mi355_png_stream *host, int nstreams)
{
    if (!host || nstreams < 1 || nstreams > 65535) return "png_inflate: null table / need 1 <= nstreams <= 65535";
    for (int s = 0; s < nstreams; ++s) {
        const char *why = pic_stream_check(&host[s]);
        if (why) return why;
    }
    return nullptr;
}

int png_inflate_launch(const mi355_png_stream *table_dev, int nstreams, int *status_dev, hipStream_t st)
{
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)nstreams), dim3(PNGI_LANES), 0, st, table_dev, status_dev);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
