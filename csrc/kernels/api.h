// C ABI of the kernel library (every function enqueues on `st` and returns the
// hipError_t of the launch; 0 = success, negative = rejected shape).
// GEMM entry points take an optional `Wsh`: the decode (M <= 64) weight in the
// skinny kernel's fragment order (ops/gemm.py shuffle_weight); nullptr = use W;
// and an optional workspace `ws` of `ws_bytes` for the decode stream kernel's
// split-K partials (nullptr: no K split).
#pragma once
#include <hip/hip_runtime.h>

extern "C" {
int dnn_gemm_bf16(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const float* bias, const void* R,
                  int ldr, int M, int N, int K, int act, int out_f32, hipStream_t st, const void* Wsh = nullptr,
                  const float* rowstat = nullptr, const float* colsum = nullptr, void* ws = nullptr,
                  long long ws_bytes = 0);
int dnn_row_stats(const void* x, int ldx, float* stats, int M, int N, float eps, int rms, hipStream_t st);
int dnn_gemm_set_tile(int tile);
int dnn_gemm_set_anatomy(int bits);
int dnn_gemm_set_skinny_pin(int id, int ks, int n, int k);
int dnn_gemm_bf16_qkv_scatter(const void* A, int lda, const void* W, int ldw, const float* bias, const float* rowstat,
                              const float* colsum, void* q, void* kc, void* vc, const int* pos, int B, int T, int H,
                              int Hkv, int hd, int S, int K, hipStream_t st);
int dnn_gemm_fp8_qkv_scatter(const void* A8, const float* sa, const void* W8, const float* sw, const float* bias,
                             void* q, void* kc, void* vc, const int* pos, int B, int T, int H, int Hkv, int hd, int S,
                             int Kb, hipStream_t st);
int dnn_gemm_set_res_prefetch(int on);
int dnn_gemm_set_half_cost(float c);
int dnn_gemm_set_skinny_max_m(int m);
int dnn_gemm_fp8_set_tile(int tile);
int dnn_gemm_fp8_256(const void* A, const float* sa, const void* W, const float* sw, void* C, int ldc, const float* bias,
                     const void* R, int ldr, int M, int N, int Kb, int act, hipStream_t st);
int dnn_gemm_skinny_sweep(const void* A, int lda, const void* W, int ldw, const float* sw, void* C, int ldc, int M,
                          int N, int K, int nt, int u, int ks, int pipe, int w8, hipStream_t st);
int dnn_gemm_skinny_norm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const float* bias,
                         const void* R, int ldr, int M, int N, int K, int act, int norm, const float* colsum, float eps,
                         hipStream_t st, const void* Wsh = nullptr, void* ws = nullptr, long long ws_bytes = 0);
int dnn_gemm_skinny_w8(const void* A, int lda, const void* W, int ldw, const float* sw, void* C, int ldc,
                       const float* bias, const void* R, int ldr, int M, int N, int K, int act, int norm,
                       const float* colsum, float eps, hipStream_t st, const void* Wsh = nullptr, void* ws = nullptr,
                       long long ws_bytes = 0);
int dnn_gemm_skinny(const void* A, int lda, const float* sa, const void* W, int ldw, const float* sw, void* C, int ldc,
                    const float* bias, const void* R, int ldr, int M, int N, int K, int act, int out_f32, int fp8,
                    hipStream_t st, const void* Wsh = nullptr, void* ws = nullptr, long long ws_bytes = 0);
// decode stream GEMM (gemm_stream.h) switch: 0 off / 1 auto / 2 forced, the weight-byte threshold (<= 0
// keeps it), and the in-launch split-K combine (fold: 1 on, 0 reduce launch, -1 keep)
int dnn_gemm_set_stream(int on, long long min_bytes, int fold = -1);
// one-shot decode GEMM (gemm_oneshot.h): on 0 off / 1 planned shapes / 2 every eligible shape; a non-zero
// (mt, ntw, steps, splitk) pins that config for every eligible call (A/B probes)
int dnn_gemm_set_oneshot(int on, int mt, int ntw, int steps, int splitk);
int dnn_gemm_set_oneshot_lds_floor(int bytes);
// race probe (gemm_oneshot.h probe bits; abl 0 = off): records per workgroup in rec
int dnn_gemm_set_oneshot_probe(void* rec, int abl);
int dnn_gemm_oneshot_sweep(const void* A, int lda, const void* Wsh, const float* sw, void* C, int ldc, int M, int N,
                           int K, int mt, int ntw, int steps, int splitk, int w8, void* ws, long long ws_bytes,
                           hipStream_t st);
// decode vocabulary head + argmax partials (gemm_head.h): returns partials per row (> 0) or < 0 (not covered)
int dnn_gemm_set_head(int on);
int dnn_gemm_head(const void* A, int lda, const void* Wsh, const float* sw, const float* colsum, const float* bias,
                  float eps, int norm, void* C, int ldc, int M, int N, int K, int w8, void* part, int part_cap,
                  hipStream_t st);
// hist (optional, with pos_inc): hist[row * hist_ld + pos_inc[row]] = id before the advance (token history)
int dnn_argmax_final(const void* part, int S, int M, int* out, int* out2, int* pos_inc, hipStream_t st,
                     int* hist = nullptr, int hist_ld = 0);
// prefill: 256^2 + 256x128 tail split (gemm_bf16.hip launch_gemm)
int dnn_gemm_set_split_tail(int on);
// MX-scaled W8A8 prefill (e8m0 per (row, 128 columns), common.h mx_index)
int dnn_quant_fp8_mx(const void* x, int ldx, void* q, int ldq, void* sx, int M, int K, int kpad, hipStream_t st);
int dnn_layernorm_q8_mx(const void* x, int ldx, const float* w, const float* b, void* q, int ldq, void* sx, int M,
                        int N, int kpad, float eps, int rms, hipStream_t st);
int dnn_gemm_fp8_mx(const void* A8, const void* sx, const void* W8, const float* sw, void* C, int ldc,
                    const float* bias, const void* R, int ldr, int M, int N, int Kb, int act, void* qo, int ldq,
                    void* sxo, int kpo, hipStream_t st);
int dnn_gemm_fp8_qkv_scatter_mx(const void* A8, const void* sx, const void* W8, const float* sw, const float* bias,
                                void* q, void* kc, void* vc, const int* pos, int B, int T, int H, int Hkv, int hd,
                                int S, int Kb, hipStream_t st);
// producer-side row statistics for the next decode GEMM call of this thread (gemm_skinny.hip)
int dnn_gemm_rowstats(void* out, int out_ld, const void* in, int in_ld);
int dnn_gemm_rowstats_written();
// decode GEMM epilogue operands with the first loads (1, default) / after (0)
int dnn_gemm_set_epi_prefetch(int on);
// probe: one-shot launch with parts removed
int dnn_gemm_oneshot_ablate(const void* A, int lda, const void* Wsh, const float* sw, void* C, int ldc, int M, int N,
                            int K, int cfg, int abl, hipStream_t st);
int dnn_silu_mul_packed(const void* gu, int ld_in, void* out, int ld_out, int M, int F, hipStream_t st);
int dnn_cifar_stage0_v4(const float* x, void* out, const void* w1p, const float* b1, const void* w2p, const float* b2,
                        int B, int grid, hipStream_t st);
int dnn_cifar_set_v4_pt(int pt);
int dnn_cifar_stage0_x3(const float* x, float* out, const void* w1h, const void* w1l, const float* b1, const void* w2h,
                        const void* w2l, const float* b2, int B, int grid, hipStream_t st, int split_out = 0,
                        const void* w1h32 = nullptr, const void* w1l32 = nullptr);
// uint8 NHWC input (B,32,32,3) normalised by table (uint32 [3][256]: bf16 hi bits low, lo bits high); K = 32
// conv1 arm only.  Negative = rejected, nothing launched: -1 null table / weights, -2 conv1 switch on K = 48,
// -3 x or table not 4-byte aligned.
int dnn_cifar_stage0_x3_u8(const unsigned char* x, const unsigned* table, float* out, const void* w1h32,
                           const void* w1l32, const float* b1, const void* w2h, const void* w2l, const float* b2, int B,
                           int grid, hipStream_t st, int split_out = 0);
int dnn_cifar_s0_set_conv1(int v);
int dnn_cifar_s0_get_conv1();
int dnn_cifar_s0_set_wide_store(int on);
int dnn_cifar_s0_get_wide_store();
int dnn_cifar_s0_set_mfma(int v);
int dnn_cifar_s0_get_mfma();
int dnn_cifar_split3(const float* a, int lda, void* o, int ldo, int M, int K, hipStream_t st, int blocked = 0);
int dnn_cifar_fc1_x3(const float* A, int lda, const void* Wh, const void* Wl, int ldw, const float* bias, float* C,
                     int ldc, int M, int N, int K, hipStream_t st, int a_split = 0);
int dnn_cifar_fc1_set_sched(int v);
int dnn_cifar_fc1_get_sched();
int dnn_cifar_split_blocked(const float* a, float* o, int M, int K, int dir, hipStream_t st);
int dnn_cifar_head_tail_x3(const float* hid, const void* w2h, const void* w2l, const float* b2, float* probs, int* pred,
                           int B, hipStream_t st);
int dnn_cifar_head_tail(const void* hid, const void* w2p, const float* b2, float* probs, int* pred, int B,
                        hipStream_t st);
// split: rows of 2 kpad bytes, e4m3 hi plane then the residual plane (W8A8 prefill with split activations)
int dnn_layernorm_q8(const void* x, int ldx, const float* w, const float* b, void* q, int ldq, float* sq, int M, int N,
                     int kpad, float eps, int rms, hipStream_t st, int split = 0);
int dnn_layernorm(const void* x, int ldx, const float* w, const float* b, void* y, int ldy, int M, int N, float eps,
                  int rms, hipStream_t st);
int dnn_embed_gpt2(const int* idx, const void* wte, const void* wpe, void* out, int B, int T, int d, const int* pos,
                   int V, int P, hipStream_t st);
int dnn_qkv_split(const void* qkv, void* q, void* kc, void* vc, int B, int T, int H, int Hkv, int hd, int S,
                  const int* pos, const float* cos, const float* sin, int rope, hipStream_t st, int kv8 = 0);
int dnn_flash_attn_qkv(const void* qkv, int ldqkv, void* kc, void* vc, void* o, int B, int T, int H, int Hkv,
                       int hd, int S, const int* pos, float scale, hipStream_t st, int kv8 = 0);
int dnn_flash_attn(const void* q, const void* kc, const void* vc, void* o, int B, int T, int H, int Hkv, int hd, int S,
                   const int* pos, float scale, hipStream_t st, int kv8 = 0);
int dnn_attn_decode_qkv(const void* qkv, int ldqkv, void* kc, void* vc, void* o, int B, int H, int Hkv, int hd, int S,
                        const int* pos, const float* cosT, const float* sinT, float scale, int splits, float* ws,
                        hipStream_t st, int kv8 = 0);
int dnn_attn_decode(const void* q, const void* kc, const void* vc, void* o, int B, int H, int Hkv, int hd, int S,
                    const int* lens, float scale, int splits, float* ws, hipStream_t st, int kv8 = 0);
int dnn_sample_topk(const void* x, int ld, int M, int N, int* out, float temperature, int topk, unsigned seed,
                    const int* step, hipStream_t st);
// temperature -> top-k -> top-p -> min-p -> draw, with the decode step tail of
// dnn_argmax_rows (sample_filter.hip); thr_out (optional): each row's final key threshold
int dnn_sample_rows(const void* x, int ld, int M, int N, int* out, float temperature, int topk, float top_p,
                    float min_p, unsigned seed, const int* step, hipStream_t st, int* out2 = nullptr,
                    int* pos_inc = nullptr, int* hist = nullptr, int hist_ld = 0, int* thr_out = nullptr);
int dnn_argmax_rows(const void* x, int ld, int M, int N, int* out, int f32in, hipStream_t st, int* out2 = nullptr,
                    int* pos_inc = nullptr, void* part = nullptr, int* hist = nullptr, int hist_ld = 0);
// repetition / presence / frequency penalties in place on bf16 logits (penalties.hip): cnt = uint16 per
// (row, entry), bit 15 "in the prompt", bits 0..14 times generated; prev (optional): the token each row
// generated last, counted first.  -1: null x / cnt, ld or cnt_ld not a multiple of 8 or below N, buffers
// not 16-byte aligned, rep not > 0, freq / pres not finite
int dnn_logit_penalties(void* x, int ld, int M, int N, unsigned short* cnt, int cnt_ld, const int* prev, float rep,
                        float freq, float pres, hipStream_t st);
// log-probability of tok[row] and the n <= 20 most likely entries (value descending, index ascending) of
// every row of bf16 logits (logprobs.hip), written at position p = pos[row] + pos_off (pos null: pos_off) of
// the histories lp_hist[row, p], top_id_hist / top_lp_hist[row, p, 0..n) (top_ld entries per position);
// p outside [0, hist_ld) writes nothing.  ws: ws_rows >= M blocks of ws_ld >= dnn_logprobs_ws_row_words(N, n)
// 32-bit words (a multiple of 32), zero before the first call; the kernel leaves each block's counter, its
// first 32 words, zero and writes nothing else there, so calls of any M, N, n may share a workspace.
// -1: null x / tok / lp_hist / ws, ld not a multiple of 8 or below N, x not 16-byte aligned, n outside
// [0, min(20, N)], top histories missing or top_ld < n, ws too small; -2: M > 65535 or N > 102 * 2048
int dnn_logprobs_ws_row_words(int N, int n);
int dnn_logprobs_rows(const void* x, int ld, int M, int N, const int* tok, const int* pos, int pos_off, int n,
                      float* lp_hist, int* top_id_hist, float* top_lp_hist, int hist_ld, int top_ld, void* ws,
                      int ws_rows, int ws_ld, hipStream_t st);
// stop tokens / stop sequences / min_new_tokens (stop.hip, which states the semantics).  state: int32
// [rows][DNN_STOP_STATE_WORDS] on the device = {g, finish length (0 = running), reason code (1 + id index,
// 17 + sequence index), the last 15 generated tokens newest first}.  The tables are HOST arrays, copied into
// the launch's arguments: stop_ids[n_ids], seqs[n_seq][DNN_STOP_MAX_SEQ_LEN] (oldest first, seq_len[s]
// entries used).  dnn_stop_rows runs behind the argmax / sampler launch on its tokens tok[M]: a finished
// row's token becomes pad in tok, also (optional) and hist[row * hist_ld + p] (optional; p = pos[row] +
// pos_off, pos null: pos_off; p outside [0, hist_ld) writes nothing); a running row counts and matches it.
// dnn_stop_suppress writes bf16 -inf into x[row, id] for every stop id of a running row with g < min_new.
// -1, nothing launched: null tok / state / x, counts above the caps, a sequence length outside 1..16, a
// negative id, pad or min_new, an id >= N (suppress), ld not a multiple of 8 or below N, x not 16-byte
// aligned; -2: M > 2^24.  M <= 0 returns 0.
#define DNN_STOP_STATE_WORDS 18
#define DNN_STOP_MAX_IDS 16
#define DNN_STOP_MAX_SEQS 8
#define DNN_STOP_MAX_SEQ_LEN 16
int dnn_stop_rows(int* tok, int* also, int* hist, int hist_ld, const int* pos, int pos_off, int* state,
                  const int* stop_ids, int n_ids, const int* seqs, const int* seq_len, int n_seq, int min_new,
                  int pad, int M, hipStream_t st);
int dnn_stop_suppress(void* x, int ld, int M, int N, const int* state, const int* stop_ids, int n_ids, int min_new,
                      hipStream_t st);
// logit constraints (constraints.hip, which states the semantics): logit_bias, allowed_token_ids,
// bad_words_ids and no_repeat_ngram_size on the bf16 logits x[M][ld] (N entries used), one launch.  ctx: int32
// [rows][ctx_ld] on the device, each row's prompt + generated tokens; len = pos[row] + pos_off (pos null:
// pos_off).  prev (optional): prev[row] in [0, N) is stored at ctx[row, len-1] first.  The tables are DEVICE
// arrays: bias_ids / bias_vals [n_bias] (distinct ids), allow = bitmask over [0, N) (bit i of byte i / 8; null =
// everything allowed; (N + 7) / 8 bytes), bad_ids [n_bad][DNN_CON_MAX_BAD_LEN] with bad_len [n_bad] entries
// used; h_* are HOST copies of the same tables, which the entry checks on every call.  -1, nothing launched:
// null x, null ctx when ngram > 0 or a bad word is longer than one token, ld not a multiple of 8 or below N, x
// not 16-byte aligned, a count above its cap, a bad-word length outside 1..16, ngram outside 0..16, a table id
// outside [0, N), a non-finite bias; -2: M > 65535.  M <= 0 returns 0.
#define DNN_CON_MAX_BIAS 256
#define DNN_CON_MAX_BAD 64
#define DNN_CON_MAX_BAD_LEN 16
#define DNN_CON_MAX_NGRAM 16
int dnn_logit_constraints(void* x, int ld, int M, int N, int* ctx, int ctx_ld, const int* pos, int pos_off,
                          const int* prev, const int* bias_ids, const float* bias_vals, int n_bias,
                          const unsigned char* allow, const int* bad_ids, const int* bad_len, int n_bad, int ngram,
                          const int* h_bias_ids, const float* h_bias_vals, const int* h_bad_ids, const int* h_bad_len,
                          hipStream_t st);
// ragged prompts (ragged.hip): one piece of a right-padded prefill covers prompt positions [t0, t0 + Tc) of B
// sequences, its bf16 hidden states h as rows (b * Tc + t) of ld entries.  For sequence b with q = lens[b] -
// 1 - t0 in [0, Tc) (its own last prompt position lies in this piece) row h[(b * Tc + q) * ld : +d] is copied
// to dst[b * dst_ld : +d]; every other dst row, and the entries of a copied row past d, keep what they hold
// (lens[b] <= 0 never matches).  -1, nothing launched: null h / lens / dst, d not a positive multiple of 8,
// Tc <= 0, t0 < 0, ld or dst_ld below d or not a multiple of 8, h or dst not 16-byte aligned; -2: B > 2^24.
// B <= 0 returns 0.
int dnn_ragged_last_rows(const void* h, int ld, const int* lens, int t0, int Tc, int B, int d, void* dst, int dst_ld,
                         hipStream_t st);
int dnn_quant_fp8_rows(const void* x, int ldx, void* q, float* scale, int M, int K, int kpad, hipStream_t st,
                       int split = 0);
int dnn_gemm_fp8(const void* A, const float* sa, const void* W, const float* sw, void* C, int ldc, const float* bias,
                 const void* R, int ldr, int M, int N, int K, int act, hipStream_t st);
}
