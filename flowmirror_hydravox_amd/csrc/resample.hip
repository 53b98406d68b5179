// resample.hip — band-limited sample-rate conversion of the prompt audio: the polyphase windowed-sinc resampler the reference runs on the host
// before anything else (cosyvoice/utils/file_utils.py:46-75, torchaudio.transforms.Resample with its default sinc_interp_hann kernel).
//
// With both rates divided by their gcd (orig, new), width = ceil(lowpass_filter_width * orig / base) and K = 2 * width + orig, output frame j holds
// `new` samples, one per phase p:
//     y[j * new + p] = sum_k h[p][k] * xpad[j * orig + k],      xpad = x with `width` zeros in front and `width + orig` zeros behind.
// The taps come from packing.sinc_resample_taps, stored phase-contiguous: taps[k * new + p].
//
// One workgroup computes a tile of `ft` consecutive frames.  It stages the xpad span of the tile, (ft - 1) * orig + K floats, in LDS once — the zero
// padding is the bounds test of that copy, there is no padded buffer — and then walks work items (phase p, frame group g): an item holds RS_FPT
// frames g, g + G, g + 2G, ... (G = ceil(ft / RS_FPT)) of one phase in registers, so every tap is loaded once for RS_FPT fp32 FMAs.
// Lanes run along p first, then g:
//   * new > 1: consecutive lanes read consecutive floats of the tap table (one coalesced row segment per k, served by L1 / L2: the table of
//     44100 -> 16000 is 304 KB) and store consecutive outputs; the lanes of a 32-lane LDS group cover 1 + 31 / new frames, i.e. that many distinct
//     LDS addresses `orig` floats apart (one address is a broadcast);
//   * new == 1: the lanes run along the frames of the tile, the tap is the same address for all of them, the outputs are consecutive, and the LDS
//     addresses of a group are `orig` floats apart.
//   ds_read_b32 banks are (address / 4) mod 32 per 32-lane group: distinct addresses `orig` apart are conflict-free for odd orig (441, 147, 3) and
//   gcd(orig, 32)-way otherwise (2-way for the orig = 2 pairs 48000 -> 24000 and 16000 -> 24000, 4-way for 32000 -> 24000) — the pairs whose K is 28
//   or less, where the whole conversion of a 30 s prompt is some ten MFLOP.
// Every output is one chain of fp32 FMAs over k ascending, whole (the zeros of the padding included): its bits do not depend on the tile it falls
// in, on ft, on the row count or on the launch.  fp32 VALU only (a 30 s prompt at 44.1 kHz is 0.23 G multiply-adds; the contract is fp32).
#include "hvx_device.h"
#include "hvx_kernels.h"

namespace hvx {

constexpr int RS_THREADS = 256;
constexpr int RS_FPT = 4;                       // frames per work item
constexpr int RS_LDS_MAX = 16384;               // floats: 64 KB, the most one workgroup may stage
constexpr int RS_LDS_AIM = 8192;                // floats: tiles are sized for 32 KB where 4 frames fit in it (more workgroups per CU, more tiles per clip)
constexpr long long RS_TAPS_MAX = 1ll << 24;    // floats: 64 MiB of taps (packing.sinc_resample_taps refuses a larger table)
constexpr long long RS_TILE_OUT_MAX = 1ll << 20;    // outputs per tile

__global__ __launch_bounds__(RS_THREADS) void resample_sinc_kernel(const float* __restrict__ x, long long x_rs, int len, const float* __restrict__ taps, int orig,
                                                                   int nw, int width, float* __restrict__ y, long long y_rs, int out_len, int ft, int span) {
    extern __shared__ float xs[];                                        // xpad[j0 * orig, j0 * orig + span)
    const int K = 2 * width + orig;
    const long long j0 = (long long)blockIdx.x * ft;                     // first frame of the tile
    const float* xr = x + (long long)blockIdx.y * x_rs;
    const long long x0 = j0 * orig - width;                              // index into x of xs[0]
    for (int i = threadIdx.x; i < span; i += RS_THREADS) {
        const long long xi = x0 + i;
        xs[i] = (xi >= 0 && xi < len) ? xr[xi] : 0.0f;
    }
    __syncthreads();
    const int G = (ft + RS_FPT - 1) / RS_FPT;
    float* yr = y + (long long)blockIdx.y * y_rs;
    for (int it = threadIdx.x; it < G * nw; it += RS_THREADS) {
        const int g = it / nw, p = it - g * nw;
        int base[RS_FPT];
        float acc[RS_FPT];
#pragma unroll
        for (int f = 0; f < RS_FPT; ++f) {
            const int fr = g + f * G;
            base[f] = (fr < ft ? fr : 0) * orig;                         // a frame past the tile reads frame 0 and stores nothing
            acc[f] = 0.0f;
        }
        const float* h = taps + p;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const float hk = h[k * nw];
#pragma unroll
            for (int f = 0; f < RS_FPT; ++f) acc[f] = fmaf(hk, xs[base[f] + k], acc[f]);
        }
#pragma unroll
        for (int f = 0; f < RS_FPT; ++f) {
            const int fr = g + f * G;
            const long long o = (j0 + fr) * nw + p;
            if (fr < ft && o < out_len) yr[o] = acc[f];
        }
    }
}

int launch_resample_sinc(const float* x, int rows, int len, long long x_rs, const float* taps, int orig, int nw, int width, float* y, int out_len,
                         long long y_rs, hipStream_t s) {
    if (!x || !taps || !y) return set_error("resample_sinc: null argument"), -1;
    if (rows <= 0 || len <= 0 || out_len <= 0 || orig <= 0 || nw <= 0 || width <= 0)
        return set_error("resample_sinc: rows %d, len %d, out_len %d, orig %d, new %d, width %d must all be positive", rows, len, out_len, orig, nw, width), -1;
    if (rows > 65535) return set_error("resample_sinc: %d rows (at most 65535 per launch)", rows), -1;
    if (x_rs < len || y_rs < out_len) return set_error("resample_sinc: row strides %lld / %lld are shorter than the rows (%d / %d)", x_rs, y_rs, len, out_len), -1;
    const long long full = ((long long)nw * len + orig - 1) / orig;      // ceil(new * len / orig)
    if (out_len > full) return set_error("resample_sinc: out_len %d exceeds ceil(%d * %d / %d) = %lld", out_len, nw, len, orig, full), -1;
    const long long K = 2ll * width + orig;
    if (K * nw > RS_TAPS_MAX) return set_error("resample_sinc: a tap table of %lld x %d floats exceeds 64 MiB", K, nw), -1;
    if (K > RS_LDS_MAX) return set_error("resample_sinc: one frame spans %lld floats (orig %d + 2 * width %d), over the 64 KB of LDS a tile may stage", K, orig, width), -1;
    // frames per tile: as many as 32 KB hold; fewer than 4 there -> up to 4 within 64 KB (one frame fits: checked above)
    long long ft = (RS_LDS_AIM - 2ll * width) / orig;
    if (ft < RS_FPT) {
        ft = (RS_LDS_MAX - 2ll * width) / orig;
        if (ft > RS_FPT) ft = RS_FPT;
    }
    const long long frames = ((long long)out_len + nw - 1) / nw;
    if (ft > frames) ft = frames;
    if (ft * nw > RS_TILE_OUT_MAX) ft = RS_TILE_OUT_MAX / nw > 1 ? RS_TILE_OUT_MAX / nw : 1;      // (keeps the kernel's item count far inside an int)
    if (ft > RS_FPT) ft = ft / RS_FPT * RS_FPT;
    const long long tiles = (frames + ft - 1) / ft;
    const long long span = ft * orig + 2ll * width;
    if (ft < 1 || span > RS_LDS_MAX || tiles > 0x7fffffffll) return set_error("resample_sinc: cannot tile %lld frames of %d (+ 2 * %d) floats", frames, orig, width), -1;
    hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)tiles, rows), dim3(RS_THREADS), (size_t)span * sizeof(float), s, x, x_rs, len, taps, orig, nw, width, y,
                       y_rs, out_len, (int)ft, (int)span);
    return hipGetLastError() == hipSuccess ? 0 : (set_error("resample_sinc launch failed"), -1);
}

}  // namespace hvx
