// hvx_kernels.h — host-side launch interface of the HIP kernels (internal to libhvx).
// Every launcher enqueues on the caller's stream, allocates nothing and never synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hvx_options.h"

namespace hvx {

// DT_F16: operands of the DiT block Linears (256-tile form only) and the activations feeding them, when the flow handle runs them in fp16; the flow's fp16
// mode (hvx_flow_config.dtype == 2) also runs the DiT attention (attention.hip: launch_dit_f16) and the position-embedding convolutions (conv_resident.hip) on it
enum DType : int { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };
inline size_t dtype_size(int dt) { return dt == DT_F32 ? 4 : 2; }

void set_error(const char* fmt, ...);

// ---- sampled per-kernel timing (bench.py: roofline.achieved) -----------------------------------------------------------
// When enabled, every `period`-th launch of a kernel class is bracketed by hipEvents on its own stream.
enum ProfKind : int { PK_SKINNY = 0, PK_GEMM = 1, PK_ATTN = 2, PK_SAMPLER = 3, PK_GEMM_F32 = 4, PK_ATTN_LLM = 5, PK_COUNT = 6 };
int prof_begin(int kind, double work, hipStream_t s);     // returns a slot (>= 0) or -1 when this launch is not sampled
void prof_end(int slot, hipStream_t s);
bool prof_enabled();

// ------------------------------------------------------------------------------------------------
// Tiled implicit-GEMM:  out[b, m, g*N + n] = epi( sum_{tap, ci} A[b, src(m, tap), g*a_gs + ci] * W[g, n, tap*cin_pad + ci] )
//   src(m, tap) = floor((m*conv_stride + tap*conv_dil - pad_left) / up), zero outside [0, rows_in*up)
// A, W are `dtype` (bf16 or f32), both K-contiguous ("NT" GEMM); accumulation is fp32 on MFMA.
// A plain Linear is taps == 1 (cin_pad == K).  Covers every Conv1d flavour of the path:
// CausalConv1d left/right (pad_left), dilation, CausalConv1dDownSample (conv_stride),
// CausalConv1dUpsample (up = nearest-neighbour factor), grouped conv (groups, a_gs).
// ------------------------------------------------------------------------------------------------
enum Epi : int { EPI_GENERIC = 0, EPI_QKV_DIT = 1 };

struct GemmArgs {
    int dtype;                    // DType of A and W
    int M, N, K;                  // per (batch, group); K % 32 == 0
    int batch, groups;
    const void* A; long long a_bs; int lda; int a_gs; int rows_in;
    int cin_pad, conv_stride, conv_dil, pad_left, up;
    const void* W; long long w_gs;            // [groups][N][K]
    int epi;
    // ---- EPI_GENERIC: v = act(acc + bias[gc]) * gate[b, gc] + res[b, m, gc] + res2[b, m, gc]; v *= scale
    //      out[b, m + out_row_off, gc] = v (f32 or dtype); out2[b, m + out2_row_off, gc] = dtype(act2(v));  gc = g*N + n
    //      (res is read at row m + res_row_off; rows whose shifted index is negative are skipped)
    const float* bias;
    int act; float act_param; const float* act_alpha;
    const float* gate; long long gate_bs;
    const float* res; long long res_bs; int ldres; int res_row_off;
    const float* res2; long long res2_bs; int ldres2;
    float scale; float div;       // v *= scale; if (div != 0) v /= div
    void* out; int out_f32; long long out_bs; int ldo; int out_row_off; int out_cols;   // cols [groups*N, out_cols) zero-filled
    void* out2; int act2; float act2_param; const float* act2_alpha; long long out2_bs; int ldo2; int out2_row_off; int out2_cols;
    // ---- EPI_QKV_DIT: N = 3*heads*64; + bias; interleaved-pair RoPE on channels [0,64) of q and k (head 0);
    //      q,k -> [b][head][t_pad][64], v -> vT [b][head][64][t_pad]   (all `dtype`)
    void* q; void* k; void* vT; int heads; int t_pad; const float* rope_cos; const float* rope_sin;   // [t][32]
    int x3;                       // fp32 operands may be split into bf16 pairs and multiplied on the bf16 matrix cores (gemm_x3.hip; ~1e-6 relative)
    float q_scale;                // != 0: q is stored multiplied by this (softmax scale * log2 e: the scores then leave the attention MFMAs in log2 units)
    // ---- fp32 values as (hi, lo) bf16 PLANE PAIRS (dtype DT_F32, x3 path): x == hi + lo up to 2^-17 |x|, hi = bf16(x), lo = bf16(x - hi).
    //      A pair is addressed like the fp32 tensor it stands for (same row / batch strides, in elements), the lo plane `*_plane` bf16
    //      elements behind the hi plane.  With a_planes and w_planes the split-bf16 GEMM reads its operands straight into LDS by LDS-DMA
    //      (gemm_x3.hip: gemm_x3p_kernel) instead of splitting fp32 values on the way in; out_planes / out2_planes make the epilogue
    //      write a pair instead of fp32 values (any fp32 GEMM form), so the next convolution finds its operand ready.
    int a_planes; long long a_plane;
    int w_planes; long long w_plane;
    int out_planes; long long out_plane;
    int out2_planes; long long out2_plane;
    // ---- HALF residual stream (DiT, bf16 mode): res and / or out hold IEEE fp16 instead of fp32 (same strides, in elements).  The reference runs
    //      its flow decoder in fp16 end to end (infer_speech_model.py:103), i.e. with an fp16 residual stream; here only the stream is fp16 — the
    //      update gate * (acc + bias) + res is formed in fp32 and rounded once on the way out.
    int res_f16; int out_f16;
    // ---- EPI_QKV_DIT with fp16 operands (gemm_big.hip): q / k / V^T are written as IEEE fp16 (round to nearest, saturated at +-65504) instead of bf16 —
    //      the attention of the flow's DT_F16 mode reads fp16
    int qkv_f16;
};
int launch_gemm(const GemmArgs& a, hipStream_t s);
int launch_gemm_x3(const GemmArgs& a, hipStream_t s);    // same convention; fp32 operands on the bf16 matrix cores (GemmArgs.x3)
int launch_conv_resident(const GemmArgs& a, hipStream_t s);   // same convention; bf16 k-tap convolutions over 64 channels per group, input rows resident in LDS (conv_resident.hip)
int launch_gemm_big(const GemmArgs& a, hipStream_t s);   // 1 = launched, 0 = not eligible (launch_gemm falls through), -1 = error

// ------------------------------------------------------------------------------------------------
// Skinny weight-streaming GEMM for the AR decode step:  out[m, n] = sum_k A[m, k] * W[n, k], M <= 128 per launch chunk.
// W is pre-packed in MFMA fragment order [N/16][K/32][64 lanes][8] so that every wave-level load is one
// contiguous 1 KiB (bf16) / 2 KiB (f32) burst.  A is row-major [M][lda].  Optional split-K writes fp32 partials.
// ------------------------------------------------------------------------------------------------
enum SkinnyEpi : int {
    SK_PARTIAL = 0,     // part[ks][m][n] = acc                                   (split-K, reduced by llm_reduce_norm)
    SK_STORE = 1,       // out[m][n] = acc + bias[n]           (f32 or dtype)
    SK_QKV_ROPE = 2,    // + bias, rotate-half RoPE, q -> qbuf, k/v -> KV cache     (llm step)
    SK_SWIGLU = 3,      // n-tiles alternate gate/up: out[m][n/2] = silu(gate) * up  (dtype)
    SK_RESID = 4,       // out[m][n] += acc + bias  (fp32 residual stream, in place; split_k == 1)
};
struct SkinnyArgs {
    int dtype;
    int M, N, K;                  // N % 16 == 0, K % 32 == 0
    const void* A; int lda;
    const void* W;                // packed
    int split_k;                  // >= 1
    int epi;
    const float* bias;
    float* part;                  // [split_k][M][N]
    void* out; int out_f32; int ldo;
    // SK_QKV_ROPE (rows are a dense [n_seq][kn] grid: m = si*kn + lt)
    int kn, q_heads, kv_heads;    // head_dim fixed at 64
    const int* slot; const int* pos0; const int* n_new;          // device [n_seq]
    const float* rope_cos; const float* rope_sin;                // [max_pos][32]
    void* qbuf;                   // [n_seq][kn][q_heads*64]              (dtype)
    void* kcache; void* vTcache;  // [slot][kv_heads][max_ctx][64] / [slot][kv_heads][64][max_ctx]   (dtype)
    int max_ctx;
    int kv_frag;                  // the caches are in fragment order (hvx_device.h: frag_index(pos, d, 2) / vfrag_index(pos, d) per (slot, kv head)); max_ctx % 32 == 0
    // layer-batched launches (MTP heads): blockIdx.z = head j, all pointers advance by these strides
    int nz; long long w_zs; long long a_zs; long long bias_zs; long long out_zs; long long part_zs;
    int n_valid;                  // SK_STORE: columns >= n_valid are not stored (0 = N)
    // fused RMSNorm (QKV / gate-up): A is the residual stream [M][lda] (dtype), W has the norm gain folded into its columns and the
    // accumulator is scaled by rsqrt(mean(x^2) + eps) per row before the epilogue
    int a_norm; float norm_eps;
    // SK_RESID: optional copy of the updated rows in `dtype` (the A operand of the next fused-norm GEMM)
    void* out2; int ldo2;
    int w_narrow;                 // SK_RESID: W is packed [N/4][K/128][64][8] (packing.pack_narrow4) for the 4-column workgroup form
    // w_narrow, one row tile (o_proj of a narrow decode grid): A is not read — its fragments are built from the key-split partials of the
    // attention launch in front (AttnArgs.part_o / part_ml with skip_combine), with the arithmetic of attn_combine_kernel, so the combine
    // launch between the two disappears.  Row m = si * kn + lt, column = q head * 64 + d; kn, q_heads, kv_heads, pos0, n_new as above.
    const float* att_o; const float* att_ml; const int* att_kvlen;
    int att_splits, att_chunk, att_rows_pad;
    // ---- wide decode grids (33..128 rows, bf16): activations in fragment order (hvx_device.h: frag_index) -----------------------
    int a_frag;                   // A is [ceil(M/16)][K/32][64][8] instead of row-major (launch_dec_gemm only)
    int out_frag;                 // SK_SWIGLU: out, SK_RESID: out2 are written in fragment order (their consumer is another launch_dec_gemm)
    // launch_dec_gemm, SK_SWIGLU: W holds e4m3 codes in double-step fragment order (packing.pack_frag_fp8; w_zs in codes) and w_scale the
    // power-of-two scale of every output column (row of W), [nz][N] with stride w_scale_zs
    int w_fp8; const float* w_scale; long long w_scale_zs;
};
int launch_skinny(const SkinnyArgs& a, hipStream_t s);
// The same GEMMs for 33..128 rows in the A-stationary / weight-ring form (gemm_dec.hip).  Returns 1 when the launch was taken, 0 when the
// shape is not one of its instantiations (the caller then uses launch_skinny on row-major activations), -1 on error.
int launch_dec_gemm(const SkinnyArgs& a, hipStream_t s);
bool dec_gemm_shape_ok(int M, int N, int K, int epi, int split_k);

// ------------------------------------------------------------------------------------------------
// Attention (flash-style online softmax, head_dim 64, one wave per (q-tile, key-split)).
// ------------------------------------------------------------------------------------------------
struct AttnArgs {
    int dtype;
    int batch, heads;             // grid.z, grid.y  (heads = kv heads when GQA-packed)
    int n_rows;                   // query rows per (batch, head) = rows_hi * kn
    int kn;                       // r -> (r_hi, r_lo) = (r / kn, r % kn)
    const void* q; long long q_bs, q_hs, q_hi, q_lo;
    const void* k; long long k_bs, k_hs;        // [.][.][key][64]
    const void* vT; long long v_bs, v_hs; int v_ld;   // [.][.][64][v_ld]
    const int* kv_slot;           // optional: batch b reads cache slot kv_slot[b]
    const int* kv_len;            // optional device [batch]; else kv_len_const
    int kv_len_const;
    int causal; const int* pos0;  // key j visible to row r iff j <= pos0[b] + r_lo  (pos0 may be null -> 0)
    const int* n_valid_lo;        // optional: rows with r_lo >= n_valid_lo[b] are skipped (inactive)
    int chunk;                    // > 0: static chunk mask (cosyvoice/utils/mask.py:128-158): row r also needs j < (r_lo / chunk + 1) * chunk
    float scale;
    int q_log2;                   // q already multiplied by scale * log2(e) (fused QKV epilogue, GemmArgs.q_scale): scale is ignored
    void* out; long long o_bs, o_hs, o_hi, o_lo;      // dtype
    int n_splits; int split_chunk;                    // keys per split (multiple of 32) when n_splits > 1
    int n_sub;                                        // waves per workgroup of that form: 4 (0 = 4), or 8 (bf16, fragment-order caches, n_rows <= 16)
    int sub_chunk;                                    // > 0 (needs n_rows <= 32): one workgroup per split, its n_sub waves take sub_chunk keys
                                                      // each and merge their (m, l, o) in LDS, so the combine reads 4x fewer partials
    float* part_o; float* part_ml;                    // [batch][heads][n_splits][n_rows_pad][64], [...][n_rows_pad][2]
    int n_rows_pad;
    int skip_combine;                                 // n_splits > 1: leave the partials to the consumer (SkinnyArgs.att_o), `out` is not written
    int kv_frag;                                      // k / vT are the LLM's fragment-order caches (hvx_device.h: frag_index(key, d, 2), vfrag_index(key, d)
                                                      // per (batch, head) block of k_hs / v_hs elements); v_ld = the cache's context capacity
    int o_frag_kt;                                    // > 0 (LLM decode, 16-bit): out is the [batch * kn][heads * rows_hi * 64] activation matrix in fragment
                                                      // order (hvx_device.h: frag_index) with this many k-steps per row; the o_* strides are ignored
    // ---- windowed DiT form (incremental streaming flow): the n_rows query rows are rows row_off .. row_off + n_rows - 1 of a sequence whose keys [0, kv_len) sit in a
    //      cache ([.][heads][v_ld][64] / [.][heads][64][v_ld], v_ld % 64 == 0, kv_len <= v_ld); the chunk mask uses the ABSOLUTE row: key j < ((row_off + r) / chunk + 1) * chunk
    const int* row_off;                               // optional device [batch]; else row_off_const (0: the rows start the sequence, every other form)
    int row_off_const;
    int window;                                       // != 0: split the keys over workgroups (attn_window_kernel for 16-bit operands, the generic kernel for fp32) and combine.
                                                      // n_splits = the most splits part_o / part_ml hold, split_chunk = keys per split (multiple of 64) or 0: chosen per launch
                                                      // from kv_len_const, which must be the LONGEST kv_len of the launch
};
int launch_attention(const AttnArgs& a, hipStream_t s);
int attention_window_splits(int dtype, int batch, int heads, int n_rows, int kv_max, int max_splits, int* split_chunk);   // the split count / length launch_attention chooses


// ------------------------------------------------------------------------------------------------
// Small fused kernels
// ------------------------------------------------------------------------------------------------
// x[m,:] += sum_s part[s][m][:] (+ bias);  y[m,:] = dtype( rmsnorm(x[m,:]) * g )          (any of part/g may be null)
//   rows are grouped in blocks of rows_per_z (MTP heads): block z uses part + z*part_zs, gain + z*gain_zs, bias + z*bias_zs.
//   do_norm == 0 -> y = dtype(x) (plain cast).
struct ReduceNormArgs {
    float* x; int ldx;
    const float* part; int split_k; long long part_stride; long long part_zs;
    const float* bias; long long bias_zs;
    const float* gain; long long gain_zs; float eps; int do_norm;
    void* y; int ldy; int dtype;
    int M, H, rows_per_z;
    int y_frag;                   // y (16-bit) is written in fragment order (hvx_device.h: frag_index, KT = H / 32)
    int y_frag_zrows;             // > 0: every z block is its own fragment-order matrix of this many (multiple of 16) rows: row = z * y_frag_zrows + m % rows_per_z
};
int launch_reduce_rmsnorm(const ReduceNormArgs& a, hipStream_t s);
// y[r, c] = dtype(act(x[r, c])) for a [rows][cols] f32 matrix (per-column alpha for Snake)
int launch_act_rows(const float* x, int ldx, void* y, int ldy, int dtype, int act, float param, const float* alpha, long long rows, int cols,
                    hipStream_t s);
int launch_act_rows_planes(const float* x, int ldx, void* y, int ldy, long long plane, int act, float param, const float* alpha, long long rows, int cols, hipStream_t s);
// gather rows: y[r,:] = x[idx[r],:] (idx[r] < 0 -> zeros)
int launch_heads_prologue(const float* x, int ldx, const int* idx, const float* gain_f, float eps_f, const float* gain_h, float eps_h, int K,
                          int S, int H, float* ylast, float* hx, void* ha, int dtype, hipStream_t s);
int launch_gather_rows_f32(const float* x, int ldx, const int* idx, float* y, int ldy, int rows, int H, hipStream_t s);
// embedding: x[r,:] = table[tok[r],:] as f32 (tok < 0 -> zeros); table dtype f32/bf16
int launch_embed(const void* table, int table_dtype, const int* tok, float* x, int ldx, int rows, int H, hipStream_t s);
// LLM input rows: tok >= 0 -> speech[tok]; tok <= -2 -> text[-tok-2]; tok == -1 -> zeros   (llm_multi_head_v3.py:941-952)
//   copy_frag: x_copy (16-bit) is written in fragment order (hvx_device.h: frag_index)
int launch_embed2(const void* speech, const void* text, int dtype, const int* tok, float* x, int ldx, void* x_copy, int rows, int H, hipStream_t s,
                  int copy_frag = 0);
// logits -> log_softmax (fp32, in place) over V columns, one block per row
// row b of the launch is row (b / grp) * grp_stride + b % grp of x: the first grp of every grp_stride rows (the live heads of a [S][K][V] block)
int launch_log_softmax(float* x, int ld, int rows, int V, hipStream_t s, int grp = 1, int grp_stride = 1);
// DiT: y = dtype( LN(x; eps, no affine) * (1 + scale[b]) + shift[b] ); x f32 [B][T][D]; shift/scale f32 [B][.] with stride mod_bs
int launch_layernorm_mod(const void* x, int x_f16, const float* shift, const float* scale, long long mod_bs, float eps, void* y, int dtype,
                         int B, int T, int D, hipStream_t s);
// DiT input: y[b,t,:] = dtype( cat[x[b,:,t], cond[b,:,t], mu[b,:,t], spk[b,:]] ), inputs f32 channel-major (B,80,T)
int launch_dit_concat(const float* x, const float* cond, const float* mu, const float* spk, void* y, int dtype, int B, int T, int mel,
                      hipStream_t s);
// sinusoidal time embedding (DiT/modules.py:71-83): y[b,:] = dtype([sin(1000 t e_i), cos(1000 t e_i)])
int launch_time_sinus(const float* t, void* y, int dtype, int B, int dim, hipStream_t s);
// CFG + Euler (flow_matching.py:116-120): x += dt * ((1+r) * v[0] - r * v[1]); v is [2][T][ldv] row-major f32, x is (80,T) f32
int launch_cfg_euler(float* x, const float* v, int ldv, long long v_bs, float dt, float rate, int T, int mel, hipStream_t s);
// generic strided f32 copy / cast helpers
int launch_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long long n, hipStream_t s);

// ---- Matcha / HiFi-GAN v1 family ----------------------------------------------------------------------
struct PackRowsArgs {
    const float* src[4]; int channels[4]; int broadcast[4];     // source k: (B, C_k, T) channel-major, or (B, C_k) broadcast over T
    float* dst; int ld; int T;                                   // dst [B][T][ld], columns beyond the sources zero-filled
};
int launch_pack_rows(const PackRowsArgs& a, int B, hipStream_t s);
size_t groupnorm_ws_bytes(int B, int T, int G);
// y = (act(GroupNorm_G(x * mask)) + tbias[b][c]) * mask, mask = [t < len[b]]; x, y f32 time-major [B][T][ld]; ws >= groupnorm_ws_bytes
int launch_groupnorm_act(const float* x, int ld, int B, int T, int C, int G, const int* len, const float* gamma, const float* beta, float eps,
                         const float* tbias, int act, float* y, int ldy, void* ws, hipStream_t s);
int launch_mask_rows(float* x, int ld, int B, int T, int C, const int* len, hipStream_t s);
int launch_euler_rows(float* x, const float* v, int ldv, float dt, int B, int T, int mel, hipStream_t s);
int launch_reflect_pad(const float* x, float* y, int L, int pad, int total, hipStream_t s);
int launch_spectral_magnitude(const float* spec, int ld, int frames, int bins, float* mag, int ld_mag, float eps, hipStream_t s);
int launch_spectral_subtract(float* spec, int ld, int frames, int bins, const float* bias, float strength, hipStream_t s);
int launch_feature_post(float* x, int ld, int rows, int cols, int post, hipStream_t s);   // 1: whisper dynamic range + affine, 2: subtract column means
int launch_overlap_add(const float* frames_buf, int ld, int frames, int n_fft, int hop, const float* wsq, float* y, int out_len, hipStream_t s);
int launch_resample_linear(const float* x, int rows, int t_in, float* y, int t_out, hipStream_t s);   // F.interpolate(mode='linear') along the last axis
// torchaudio.transforms.Resample (sinc_interp_hann) of `rows` waveforms (resample.hip): taps [2 * width + orig][nw] from packing.sinc_resample_taps, phase contiguous
int launch_resample_sinc(const float* x, int rows, int len, long long x_rs, const float* taps, int orig, int nw, int width, float* y, int out_len, long long y_rs,
                         hipStream_t s);
int launch_transpose_f32(const float* src, float* dst, int rows, int cols, int ld_src, int ld_dst, hipStream_t s);   // dst[c][r] = src[r][c]
int launch_rows_to_dtype(const float* src, int ld_src, void* dst, int dst_dtype, int ld_dst, int rows, int cols, int cols_pad, hipStream_t s);
// Streaming mel caches (hvx_cfm_solve_stream_batch): frames [covered[i], t_len[i]) of the `mel` rows of x[i] ((n, mel, t_max) f32) go to columns
// [cache_fill[i], ...) of session i's cache plane cache[i] ((mel, cache_ld[i]) f32).  All per-session arrays are HOST arrays: the values travel by value in an
// argument block of MEL_APPEND_MAX sessions, more sessions are further launches.  check_...: 0, or -1 with the error set; nothing is launched by it.
#define MEL_APPEND_MAX 16
struct MelAppendArgs {
    const float* x; int mel, t_max;
    float* cache[MEL_APPEND_MAX];
    int t_len[MEL_APPEND_MAX], covered[MEL_APPEND_MAX], ld[MEL_APPEND_MAX], fill[MEL_APPEND_MAX];
};
int check_mel_cache_append(const char* who, int n, int mel, int t_max, const int* t_len, const int* covered, float* const* cache, const int* cache_ld,
                           const int* cache_fill);
int launch_mel_cache_append(const float* x, int n, int mel, int t_max, const int* t_len, const int* covered, float* const* cache, const int* cache_ld,
                            const int* cache_fill, hipStream_t s);
// Window K / V^T of the QKV epilogue ([entries][heads][t_pad][64] / [entries][heads][64][t_pad], entries = 2 i + branch) -> rows / columns [r0[i], r0[i] + rows[i]) of session
// i's caches: dk[i] / dv[i] point at branch 0's [heads][cap[i]][64] / [heads][64][cap[i]], branch 1's lie bs[i] elements behind.  Host arrays, by value; es = bytes per element.
struct KvAppendArgs {
    const void* k; const void* vT; int es, heads, t_pad, n;
    void* dk[MEL_APPEND_MAX]; void* dv[MEL_APPEND_MAX];
    long long bs[MEL_APPEND_MAX];
    int cap[MEL_APPEND_MAX], r0[MEL_APPEND_MAX], rows[MEL_APPEND_MAX];
};
int launch_kv_window_append(const KvAppendArgs& a, hipStream_t s);       // refuses (before launching) rows that leave a cache

// ------------------------------------------------------------------------------------------------
// Sampler (common.py:138-166 + llm_multi_head_v3.py:151-166, 890-900)
// ------------------------------------------------------------------------------------------------
struct SampleArgs {
    int n_seq, head_k, V, Vs;               // V = vocab (speech + stop ids), Vs = speech_token_size
    const float* logp; long long logp_ss, logp_hs;     // [n_seq][head_k][V]
    const int* hist; long long hist_ss; const int* hist_len;     // token history per seq (snapshot = first hist_len[s])
    const int* min_len;                     // per seq: head j ignores EOS while hist_len + j < min_len
    const int* active;                      // optional per seq (0 -> skip)
    int top_k; float top_p; int win_size; int rep_thresh;   // rep_thresh = ceil(win_size * tau_r) computed on the host in double
    const float* noise; long long noise_ss; int noise_len;  // Exp(1) stream per seq: ring of noise_len values, index = position % noise_len
    const long long* noise_limit;           // optional per seq: positions < limit are valid (absent: the plain window [0, noise_len))
    long long* cursor;                      // in/out per seq: next unread noise value
    int* out_ids;                           // [n_seq][head_k]; -1 = max_trials exhausted, -2 = noise exhausted (cursor unchanged)
    int max_trials;
    // optional per-sequence sampling parameters, [n_seq] each, all four or none (none: the scalars above serve every sequence).  The kernel
    // clamps seq_top_k to [1, MAX_CAND] itself: a device array cannot be validated at launch.
    const int* seq_top_k; const float* seq_top_p; const int* seq_win; const int* seq_thresh;
    // optional per-sequence head count, [n_seq] (NULL: head_k for everybody).  Sequence s samples heads j < clamp(seq_heads[s], 1, head_k) only; the
    // others consume no noise, their log-prob rows are never read and their out_ids entries are -3 ("no head").
    const int* seq_heads;
};
int launch_ras_sample(const SampleArgs& a, hipStream_t s);

// Between two decode steps (llm_multi_head_v3.py:890-905 and the feedback of inference_wrapper): accept the sampled ids, append
// them to the utterance and the repetition window, decide whether the sequence stops, and write the next step's tok / ctrl.
struct AdvanceArgs {
    int n_seq, head_k, win_cap, max_out, speech_tokens;
    const int* ids;                         // [n_seq][head_k] from the sampler
    int* tok; int* ctrl;                    // next step's [n_seq][head_k] tokens and [5][n_seq] control
    int* hist; int* hist_len; int* min_adj; int* active;
    int* seq_state;                         // [n_seq][8]: pos, out_len, done, min_len, max_len, steps, err, -
    int* out_tokens;                        // [n_seq][max_out]
    // optional per-sequence sampling parameters (SampleArgs: seq_*).  With them a sequence's repetition ring is seq_win[i] entries long
    // (clamped to [1, win_cap]) instead of win_cap: the ring then holds exactly the window the sampler counts over, wrapped or not.
    int* seq_top_k; float* seq_top_p; int* seq_win; int* seq_thresh;
    // optional per-sequence head count (SampleArgs: seq_heads): a sequence accepts at most clamp(seq_heads[i], 1, head_k) ids per step; the row
    // stride of ids / tok stays head_k
    int* seq_heads;
};
// the four per-sequence sampling values a joining sequence brings along (written by the join kernel beside the rest of the slot's state)
struct SeqSampling {
    int top_k; float top_p; int win_size; int rep_thresh;
};
int launch_decode_advance(const AdvanceArgs& a, hipStream_t s);
int launch_decode_join(const AdvanceArgs& a, long long* cursor, int slot, int first_tok, int pos, int min_len, int max_len, hipStream_t s,
                       const SeqSampling* q = nullptr, int heads = 0);      // heads > 0: the slot's head count, written to a.seq_heads[slot]

// the caller retires slot `slot` (a cancelled request): uses n_seq, head_k, tok, ctrl, active and seq_state of `a` only
int launch_decode_leave(const AdvanceArgs& a, int slot, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// HiFT source / STFT / iSTFT
// ------------------------------------------------------------------------------------------------
// frame-level harmonic phases (generator.py:233-260): phase[t][h] = 2*pi*480*cumsum_t( (f0[t]*(h+1)/sr) % 1 )
int launch_hift_phase(const float* f0, float* phase, int T, int H, float sr, int up, hipStream_t s);
// per-sample source (generator.py:289-317, 358-375): s[n] = tanh( sum_h w[h]*(sin(phase[t][h])*amp*uv + namp*table[n][h]) + b )
int launch_hift_source(const float* f0, const float* phase, const float* table, const float* w, const float* b, float* s_out,
                       int T, int H, int up, float amp, float sigma, float vthr, hipStream_t s);
// the streaming vocoder (hvx_hift_stream_piece): the phase scan continued over frames [t_a, t_b) from the double sums carried in sums[H] (read when
// t_a > 0, rewritten with the sums after frame t_b - 1); f0 / phase are the stream state's arrays, indexed by absolute frame; counters[0..1] = t_b, samples
int launch_hift_phase_continue(const float* f0, float* phase, double* sums, long long* counters, int t_a, int t_b, int H, float sr, int up,
                               long long samples, hipStream_t s);
// ... and the source of the absolute samples [n0, n1) from those arrays, table[n][h] addressed by absolute sample; s_out[n - n0]
int launch_hift_source_window(const float* f0, const float* phase, const float* table, const float* w, const float* b, float* s_out,
                              long long n0, long long n1, int H, int up, float amp, float sigma, float vthr, hipStream_t s);
// STFT n_fft=16 hop=4 hann, center/reflect (generator.py:491-497): spec[f][0..8]=re, [9..17]=im, row stride ld (>=18, rest zero)
int launch_hift_stft(const float* s_in, float* spec, int L, int ld, hipStream_t s);
// x[f][0..8] -> mag=exp clip 1e2, x[f][9..17] -> phase=sin; iSTFT; clamp (generator.py:702-710, 499-505)
int launch_hift_istft(const float* x, int ld, float* wav, int frames, float limit, hipStream_t s);
// reflection pad (1,0) on a time-major buffer: row0 = row2 (generator.py:686-687)
int launch_copy_row(float* buf, int ld, int dst_row, int src_row, int cols, hipStream_t s);

}  // namespace hvx
