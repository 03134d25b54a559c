// Host-side launchers of the gfx950 kernels (one definition per .hip file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace nd {

struct GemmArgs {
  const float* A = nullptr;
  int lda = 0;
  const float* W = nullptr;  // [N, K] row-major (torch Linear layout)
  int ldw = 0;
  const float* bias = nullptr;
  const float* R = nullptr;  // residual [M, N]
  int ldr = 0;
  float* C = nullptr;
  int ldc = 0;
  // LayerNorm prologue over K (K == 256): rows of A are normalised,
  // (a - mean) * rstd; the LayerNorm's affine (gamma, beta) is folded into
  // W and bias once at load time (launch_fold_layernorm).
  bool norm = false;
  int M = 0, N = 0, K = 0;
  bool relu = false;
  // Row statistics hand-off (LayerNorm fusion across kernels):
  //  part_out: the producer writes, per output row and per column tile j of
  //            width N/part_n, {mean_j, M2_j} (M2 = sum of squared deviations)
  //            at part_out[(row*16 + j)*2]; launch_gemm reports part_n.
  //  part_in:  the LN consumer merges part_n_in such partials per row (Chan's
  //            formula) instead of re-reading and reducing the row.
  float* part_out = nullptr;
  const float* part_in = nullptr;
  int part_n_in = 0;
  int part_n_out = 0;  // set by launch_gemm
  // split-fp16 operand path (row-major kernel only): W pre-split by
  // launch_split_weight into fp16 hi/lo planes scaled by 2^s; the product is
  // computed as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 and the
  // accumulator scaled back by wscale = 2^-s (exact).
  const uint16_t* Wh = nullptr;
  float wscale = 1.0f;
  // P16 GEMMs: the weight's row-major split image too (large-M route through
  // the LDS-tiled kernel, launch_gemm_p16), and the P16 operand mode of the
  // row-major kernel (A, R, C in P16; lda / ldr / ldc unused)
  const uint16_t* Wh_rm = nullptr;
  float wscale_rm = 1.0f;
  int p16io = 0;
  int xcd_map = 0;     // row-major kernel: XCD-aware tile order (set by launch_gemm)
  int xcd_a = 0;       // P16 kernel: row-block split over the 8 XCDs (0: grid order; set by launch_p16)
  // split-fp16 range guard (common.hpp flag_overflow): set to 1 when a split
  // activation operand (no LN prologue) reaches |x| >= 65504; nullable
  int* ovf = nullptr;
  // --fast beam: row r belongs to chunk r / skip_rpc; a tile whose rows all
  // belong to finished chunks (skip[chunk] != 0) exits without work; nullable
  const int* skip = nullptr;
  int skip_rpc = 1;
  // P16 GEMMs: stay on the small-M kernels at any M (the beam loop's tail,
  // when few chunks are alive: a 16-row block's latency, not a 64-row tile's)
  int prefer_p16 = 0;
  // P16 GEMMs: C written row-major [M16][N] instead of P16 (the memory-bank
  // kernel's q': its one-row-per-chunk loads then read whole 1 KB runs, not
  // 16 B of every 64 B line; PMC: 4x over-fetch of q' in the P16 layout)
  int c_rm = 0;
  // row-major LDS-tiled kernel, N = layers * 512 (the beam's context K / V):
  // write the 24-bit image instead of C: layer l's row r at q24 + l *
  // q24_plane + r * CTXQ_ROW (layer-major planes, launch_ctx_pack_q24); nullable
  uint8_t* q24 = nullptr;
  size_t q24_plane = 0;
  // P16 GEMMs at K >= 1024: the split-K form's fp32 slab and per-tile tickets
  // (zero before the first launch; the last arriver of a tile resets its
  // ticket), sized for sk_tiles 32 x 32 tiles; null: the one-workgroup form
  float* sk_slab = nullptr;
  int* sk_cnt = nullptr;
  int sk_tiles = 0;
};
#define ND_PART_LD 16  // partial-stat slots per row (max column tiles of a 256-wide row)
// row-major operands (encoder, large M): LDS-tiled MFMA kernel
hipError_t launch_gemm(GemmArgs& g, hipStream_t s);
// P16-packed operands (decoder steps, small M; common.hpp pk()): A, W, R, C
// packed, lda/ldw/ldr/ldc ignored, rows padded to a multiple of 16 in every
// buffer (part buffers included); LN requires part_in.
hipError_t launch_gemm_p16(GemmArgs& g, hipStream_t s);
// W [N, K] fp32 (leading dimension ld) -> Wh (split-fp16, [N][K/8][hi 8 | lo 8] halves) with the
// power-of-two scale that puts max|W| just under 2^14; returns 2^-s in
// *wscale (synchronises the stream: load-time only).  K % 32 == 0.
hipError_t launch_split_weight(const float* W, int ld, int N, int K, uint16_t* Wh, float* wscale, hipStream_t s);
// P16H image of a row-major weight [N, K] (leading dim ld) for the split-fp16
// P16 kernels: [N/16][K/32][hi | lo][64 lanes][8 halves] of W * 2^s (scale as
// launch_split_weight; synchronises the stream).  N % 16 == 0, K % 32 == 0.
hipError_t launch_pack_p16h(const float* W, int ld, int N, int K, uint16_t* out, float* wscale, hipStream_t s);
// launches per GEMM route (include/nanodec.h ND_ROUTE_*) since the last reset
long long gemm_route_count(int route, bool reset);
// raises the dynamic-LDS limit of the LDS-staged GEMM kernels (once per process)
hipError_t init_gemm_attributes();
// row-major [M, N] with leading dimension ld -> P16 (M, N multiples of 16)
hipError_t launch_pack_p16(const float* src, int ld, float* dst, int M, int N, hipStream_t s);
// W_out[n][k] = W[n][k] * ln_g[k];  b_out[n] = bias[n] + sum_k W[n][k] * ln_b[k]
// (LayerNorm(x) W^T + b == xhat (W diag(g))^T + (W beta + b)); bias may be null.
hipError_t launch_fold_layernorm(const float* W, const float* bias, const float* ln_g, const float* ln_b,
                                 float* W_out, float* b_out, int N, int K, hipStream_t s);

// Launch arguments: host-only aggregates filled by field name; the launchers unpack them into the kernels'
// argument lists.  (GemmArgs, EncWo, EncQkv, DecFfn and R2Args are kernel arguments themselves, passed by value:
// their member order and types are the kernels' layout.)
// the source-side key mask: keys t < span[c], those with signal[c*T + t] == pad_val filled with ND_MASK_FILL
struct SrcMask {
  const float* signal = nullptr;
  const int* span = nullptr;
  float pad_val = 0.f;
};

// ---- encoder -------------------------------------------------------------
// Layer 0 of the Transformer encoder reads x = s w + b (Linear(1, d) of the
// sample s): with w' = w - mean(w), b' = b - mean(b) its LayerNorm'd
// projection is the rank-2 form, written about the variance's minimum
// s0 = -mean(w'b') / mean(w'^2) (rounded to fp32; 0 while cos^2(w', b') <=
// 1/16, embed_qkv_prep_kernel), s' = s - s0, and b_perp = b' + s0 w' (so
// s w' + b' = s' w' + b_perp exactly):
//   LN(x) W'^T + b'' = (s' a + c) / sqrt(s'^2 m_ww + 2 s' m_wb + m_bb + eps) + b''
// a = W' w', c = W' b_perp, m_.. the means of w'^2, w' b_perp (0 up to s0's
// rounding), b_perp^2 (W', b'': the LN-folded QKV weight and bias), so the
// layer needs no QKV GEMM.  About s = 0 instead (c = W' b', the means of b')
// the variance's minimum m_bb - m_wb^2 / m_ww and then s a + c both cancel
// when w' and b' are nearly collinear (tests/test_enc_layer0_scheme.py);
// b_perp is orthogonal to w', so neither does here.
struct EmbedQkv {
  const float* ac = nullptr;  // [2][768]: a, c
  const float* bias = nullptr;
  float mww = 0.f, mwb = 0.f, mbb = 0.f;
  float s0 = 0.f;
  float* qkv = nullptr;       // unread (the rows are never materialised); keeps R2Args' kernel-argument layout
};
// Layer 0's attention in the same closed form: per head h the query, key
// and value of position t are u_h y_t + v_h r_t + w_h (y = s r, r the LN
// scale of the row), so a score is y_u alpha_t + r_u beta_t + (a constant
// of t that cancels in the softmax) with alpha_t, beta_t linear in
// (y_t, r_t, 1) (coef [8 heads][6], log2 units; y = s' r), and the output is
// a_v E[y] + c_v E[r] + b_v over the softmax: out [M, 256] row-major.
struct R2Args {
  const float* signal = nullptr;
  const int* span = nullptr;
  EmbedQkv eq;
  const float* coef = nullptr;
  float* out = nullptr;
};
hipError_t launch_enc_attention_rank2(const R2Args& a, int B, int T, hipStream_t s);
// ac and the scalars (double scal[4]: the three means and s0) from the LN-folded weight [768, 256]
hipError_t launch_embed_qkv_prep(const float* w_in, const float* b_in, const float* nwqkv, float* ac, double* scal,
                                 hipStream_t s);
// Layer 0's whole load-time preparation, for nd_finalize and nd_op_enc_layer0 alike: the prep launch into ac
// [6][256] and scal [4], the 48 coef values (computed in double on the host) into coef, all three on the device,
// and *eq filled for launch_enc_attention_rank2.  Synchronises s.
hipError_t prepare_embed_qkv(const float* w_in, const float* b_in, const float* nwqkv, const float* nbqkv, float* ac,
                             double* scal, float* coef, EmbedQkv* eq, hipStream_t s);
// x[b*T+t][:] = signal[b][t] * w_in + b_in (Linear(1, d)); part: full-row stats
hipError_t launch_enc_embed(const float* signal, const float* w_in, const float* b_in, float* x, float* part, int B,
                            int T, hipStream_t s);
// flash attention over qkv [B*T, 768]; mask: signal == 0 (pad_val is not read), keys >= span excluded.
// 1 <= span[b] is required: the split-fp16 kernel clamps its row loads to span - 1 (span = 0 would read the
// row before the chunk); rows at or past span are read by neither form for their values.
struct EncAttnArgs {
  const float* qkv = nullptr;
  SrcMask mask;
  float* out = nullptr;
  int B = 0, T = 0;
  bool exact = false;  // the fp32-MFMA kernel instead of split-fp16
  int* ovf = nullptr;  // split-fp16 range guard word (nullable)
};
hipError_t launch_enc_attention(const EncAttnArgs& a, hipStream_t s);
// NanoEncoder BiLSTM layer (both directions): xp [B*T, 1024] projections
// (or, layer0, computed from signal with wih0/bsum [2][512]); whh [2][512][128];
// out [B*T, 256] (h, or BatchNorm(h) when bn_scale != nullptr).
struct LstmArgs {
  const float* xp = nullptr;
  const float* signal = nullptr;
  const float* wih0 = nullptr;
  const float* bsum = nullptr;
  const float* whh = nullptr;
  const int* len = nullptr;
  int B = 0, T = 0;
  float* out = nullptr;
  const float* bn_scale = nullptr;
  const float* bn_shift = nullptr;
  bool layer0 = false;
  bool exact = false;  // fp32 MFMAs instead of split-fp16
};
hipError_t launch_lstm_layer(const LstmArgs& a, hipStream_t s);
// fused encoder FFN block (ffn.hip): x = y + W2 relu(W1' LN(y) + b1') + b2 with
// the LN affine folded into W1' / b1'; w1h = P16H image of W1' [F, 256], w2h =
// P16H image of W2 [256, F] (launch_pack_p16h), w*s their scales; xpart gets
// each row's exact {mean, M2} in slot 0 (one partial).  F % 32 == 0, F <= 2048.
struct FfnArgs {
  const float* y = nullptr;
  const uint16_t* w1h = nullptr;
  float w1s = 1.f;
  const float* b1 = nullptr;
  const uint16_t* w2h = nullptr;
  float w2s = 1.f;
  const float* b2 = nullptr;
  float* x = nullptr;
  float* xpart = nullptr;
  int M = 0, F = 0;
  int* ovf = nullptr;  // split-fp16 range guard word (nullable)
};
// wo (att == nullptr: none): the attention block's output projection folded in
// front, y = x + att Wo^T + bo with y the residual argument (x may alias it),
// woh the P16H image of Wo [256, 256], wos its scale.
struct EncWo {
  const float* att = nullptr;
  const uint16_t* woh = nullptr;
  float wos = 1.f;
  const float* bo = nullptr;
};
// qk (wh == nullptr: none): the NEXT layer's QKV projection folded behind, out = LN(x)
// W'^T + b' (wh: P16H image of the LN-folded W' [768, 256], ws its scale;
// out row-major [M, 768])
struct EncQkv {
  const uint16_t* wh = nullptr;
  float ws = 1.f;
  const float* bias = nullptr;
  float* out = nullptr;
};
hipError_t launch_enc_ffn(const FfnArgs& a, EncWo wo, EncQkv qk, hipStream_t s);
// The same block for the beam's decoder rows (P16-packed y and x, the layer's
// position_ffn.py:27-40 at decoder/transformer.py:92): the d_ff walk split
// over nsplit workgroups per 128-row block (blockIdx.y), whose partial
// accumulators meet in an fp32 slab; the workgroup that draws a row block's
// last ticket sums them in split order (deterministic), adds nothing else
// (b2 and the residual are split 0's initial value) and writes x and the
// rows' exact statistics.  Row blocks whose chunks are all done (skip) exit.
struct DecFfn {
  int nsplit = 1;
  float* slab = nullptr;    // [row block][split][16 tiles][512 threads] f32x4
  int* tickets = nullptr;   // [row block], zero between launches
  const int* skip = nullptr;
  int skip_rpc = 1;
};
size_t dec_ffn_slab_floats(int M, int nsplit);
hipError_t launch_dec_ffn(const FfnArgs& a, const DecFfn& df, hipStream_t s);
// out[r] = LN(x[r]) (rows of 256)
hipError_t launch_layernorm(const float* x, const float* g, const float* b, float* out, int rows, hipStream_t s);

// ---- decoder -------------------------------------------------------------
// Layer 0's self-attention reads its row's q | k | v from the model's table
// QKV0[step][token] ([S * V, 768]; launch_dec_embed_table + one GEMM, built
// once at finalize) instead of a per-step GEMM: its input LN(emb[tok] * 16 +
// pe[step]) takes only V values per step.  tok == nullptr: the per-step qkv
// matrix.
struct QkvRows {
  const int* tok = nullptr;  // row -> token of this step (steps > 0)
  int V = 0;
  int tok0 = 0;  // every row's step-0 token (BOS)
  // q | k | v (the table or the per-step matrix) row-major [rows][768]
  // instead of P16: a workgroup reads ONE row, which in P16 is 16 B of every
  // 128 B line (GemmArgs.c_rm)
  int rm = 0;
  // Table history (greedy rows: one row per chunk, no ancestry, no skip list,
  // fp32, row-major table): hist[r * hist_ld + t] is row r's token picked at
  // step t (the greedy head's out_tokens), so key t < step of row r is the
  // k | v part of table row t * V + (t == 0 ? tok0 : hist[r][t - 1]) and the
  // kernel neither reads nor writes the cache.  nullptr: the cache.
  const int* hist = nullptr;
  int hist_ld = 0;
};
// rows s * V + v (s < S, v < V) of the layer-0 QKV table's input, P16, with
// one row-statistics partial per row; rows S * V .. rows_alloc - 1 zero
hipError_t launch_dec_embed_table(const float* emb, const float* pe, int V, int S, float* x, float* part, int rows_alloc,
                                  hipStream_t s);
hipError_t launch_dec_embed(const int* tok, const float* emb, const float* pe, int step, float* x, float* part,
                            int R, hipStream_t s);
hipError_t launch_fill_i32(int* p, int v, int n, hipStream_t s);
// raises the dynamic-LDS limit of every form of the decoder attentions and the GEMMs (once per process)
hipError_t init_kernel_attributes();

// Two more bundles recur in the decoder-step launch arguments (with SrcMask, above):
// the chunks and rows a launch covers: rows r = c * rpc + j of the chunks c < C
struct RowSet {
  int C = 0;
  int rpc = 1;
  const int* done = nullptr;   // --fast beam: per chunk, nonzero = finished, its rows do nothing
  // --fast beam tail: the launch runs the chunks listed here only (ccap entries, -1 = none);
  // launch_alive_list builds the list from the done flags
  const int* clist = nullptr;
  int ccap = 0;
};
// kernel stamps (common.hpp stamp_begin) and the -attn_debug capture of the head-0 scores
struct AttnTap {
  unsigned long long* stamp = nullptr;
  float* dbg = nullptr;
  size_t dbg_stride = 0;
};
// self attention: writes k,v of this step into cache[slot=r][step], attends
// over the row's history cache[anc[r][t]][t] (anc == nullptr: identity).
// qr.hist (table history, QkvRows): the history comes from the table, the cache is not touched.
struct GreedyHead;
struct SelfAttnArgs {
  const float* qkv = nullptr;
  float* cache = nullptr;
  const int* anc = nullptr;
  int anc_ld = 0, step = 0, max_steps = 0;
  float* out = nullptr;
  int R = 0;    // rows of qkv and out
  RowSet rows;  // rpc, done and the chunk list (C unused: R says it)
  QkvRows qr;
  // greedy, table history, step > 0: the workgroup of row r first runs the previous step's greedy head
  // for r (its token is this step's input), so the standalone head kernel runs only after the last step
  const GreedyHead* head = nullptr;
  bool q24 = false;  // the cache holds 1600-B 24-bit rows (attention.hip SELF_Q24_ROW) instead of [512] floats
};
hipError_t launch_dec_self_attention(const SelfAttnArgs& a, hipStream_t s);
// context attention: rows r = c*rpc + j attend over ctxkv rows of chunk c
// (K at kv[(c*T+t)*ld + koff], V at +256)
struct CtxAttnArgs {
  const float* q = nullptr;
  const void* kv = nullptr;
  int ld = 0, koff = 0;
  bool q24 = false;  // kv is the 24-bit image of launch_ctx_pack_q24 (ld, koff in bytes)
  int T = 0;
  float* out = nullptr;
  SrcMask mask;
  RowSet rows;
  AttnTap tap;
  int nsplit = 1;         // workgroups per listed chunk (rows.clist; the -attn_debug form runs whole)
  float* part = nullptr;  // nsplit > 1: scratch of ccap * nsplit * rpc * (256 + 16) floats
};
hipError_t launch_dec_ctx_attention(const CtxAttnArgs& a, hipStream_t s);
// RowSet.clist from the done flags (*ovf = 1 when more than cap are alive)
hipError_t launch_alive_list(const int* done, int C, int* list, int cap, int* ovf, hipStream_t s);
// 24-bit context K/V (beam rows): per (key row, layer) CTXQ_ROW bytes = k's 256
// integers (3 bytes each, lane i's 12 bytes = dims 4i..4i+3) | v's | per head
// {k scale, v scale} (powers of two, f32).  Image [Ld][B*T][CTXQ_ROW] (layer-
// major: one layer's keys of a chunk are one contiguous 819 KB run, round 5)
// from the fp32 [B*T][ld] K/V (layer l at column l*512); rows t >= span not
// written.
#define CTXQ_V 768
#define CTXQ_S 1536
#define CTXQ_ROW 1600
hipError_t launch_ctx_pack_q24(const float* kv, int ld, int Ld, uint8_t* out, const int* span, int B, int T,
                               hipStream_t s);
// Next step's decoder input, written by the search kernel that picks the
// token (the embedding of step+1 fused into the head: one launch fewer per
// step): x[row] = emb[tok] (* 16 + pe[step+1] with position encoding) and
// its row statistics.  Skipped after the last step.
struct NextEmbed {
  const float* emb = nullptr;
  const float* pe = nullptr;  // null: no position encoding (and no sqrt(d) scale)
  float* x = nullptr;
  float* part = nullptr;
  int* tok = nullptr;  // optional: the row's token (the layer-0 QKV table's row index)
};
// memory-bank context attention (greedy, one row per chunk: rpc == 1):
// qp = Q' [C, 8*256] P16 (column block h = head h's 256-dim query in memory
// space), mem = row-major memory bank [C * ldT, 256] (chunk c's position t at
// row c*ldT + t, t < T <= ldT); out = U [C, 8*256] P16 (head h's
// softmax-weighted memory sum).
struct MemAttnArgs {
  const float* qp = nullptr;
  const float* mem = nullptr;
  SrcMask mask;
  float* out = nullptr;
  int C = 0, rpc = 1, T = 0, ldT = 0;
  AttnTap tap;
  int grid = 0;  // workgroups at most (they walk the chunks); 0 = one per chunk
};
hipError_t launch_dec_mem_attention(const MemAttnArgs& a, hipStream_t s);
// -attn_debug: raw head-0 score rows [B*S][T] (keys < span[c]) -> probabilities
hipError_t launch_attn_rows_softmax(float* a, const int* span, int B, int S, int T, hipStream_t s);
// stamp pairs (earliest start, latest end) <- (UINT64_MAX, 0)
hipError_t launch_stamp_reset(unsigned long long* stamps, int pairs, hipStream_t s);
// encoder output rows x[b*T+t] -> memory bank rows b*ldT+t, row-major (LN when
// ln_g; rows t >= T of each chunk zero)
// the 24-bit digit bank serves T in [1, 512] (the context's bank buffer holds 512 rows per chunk)
bool bank_eligible(int T, int ldT);
hipError_t launch_memory_pack(const float* x, const float* ln_g, const float* ln_b, float* out, int B, int T, int ldT,
                              hipStream_t s);
hipError_t init_mem_attributes();
// 24-bit fixed-point memory bank (bank8.hip): digits in bank (B * 512 * 256 * 3
// bytes), per-row scales kscale [B * 512], per-chunk biased max exponent kemax [B]
// from the encoder output rows x [B*T, 256] (LN when ln_g; keys >= span zero); ovf: a non-finite row (nullable)
struct BankPackArgs {
  const float* x = nullptr;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  void* bank = nullptr;
  float* kscale = nullptr;
  int* kemax = nullptr;
  const int* span = nullptr;
  int B = 0, T = 0;
  int* ovf = nullptr;
};
hipError_t launch_bank_pack_d8(const BankPackArgs& a, hipStream_t s);
struct BankD8Args {
  const float* qp = nullptr;  // [C, 8*256] row-major
  const void* bank = nullptr;
  const float* kscale = nullptr;
  const int* kemax = nullptr;
  SrcMask mask;
  float* out = nullptr;
  int C = 0, T = 0;
  AttnTap tap;
  int* ovf = nullptr;
  bool nt = false;  // stream the bank with non-temporal loads
  int grid = 0;     // as MemAttnArgs.grid
};
hipError_t launch_dec_bank_d8(const BankD8Args& a, hipStream_t s);
hipError_t init_bank8_attributes();
// signal front end (frontend.hip): per-read normalisation (method 0 none, 1
// median/MAD, 2 median/std; fp64 math, float32 out) of reads concatenated at
// off[0..R], and windowing of chunks (read, start, len) into a [C, T] batch
hipError_t launch_read_normalize(const double* raw, const long long* off, int R, int method, float* out,
                                 hipStream_t s);
hipError_t launch_read_window(const float* sig, const long long* off, const int* rd, const int* start,
                              const int* len, int C, int T, float* out, hipStream_t s);
// read assembly (assembly.hip): the overlap consensus of utils/labelop.py:310-352 for R reads whose chunk
// strings (ASCII, spaces removed) are concatenated in bases[total].  The optional pairs are given both or
// neither; mw / ml only beside qw / qual, bp / rpos only without them.
struct AsmArgs {
  const unsigned char* bases = nullptr;
  const int* chunk_off = nullptr;  // chunk c = bases[chunk_off[c] .. chunk_off[c+1])
  const int* read_off = nullptr;   // read r = chunks read_off[r] .. read_off[r+1]
  int R = 0, C = 0, total = 0;
  unsigned char* seq = nullptr;  // read r's bases, at chunk_off[read_off[r]]
  int* seq_len = nullptr;        // their count; -1 when status[r] != 0: the read was not assembled
  int* status = nullptr;         // bit 0: a chunk of 200 or more chars, bit 1: a char outside ACGTM
  void* work = nullptr;  // assemble_work_bytes(C, total, qual, ml, rpos given) bytes, 8-byte aligned
  const unsigned short* qw = nullptr;  // each base's uint16 weight
  unsigned char* qual = nullptr;       // the columns' qualities Q in 0..40, laid out like seq
  const unsigned short* mw = nullptr;  // each base's uint16 modification weight
  unsigned char* ml = nullptr;  // min(255, (256 W) div (65535 n_cm)) of a column called C or M (W the mw sum of
                                // its C and M votes, n_cm their number), every other byte 0; laid out like seq
  const unsigned* bp = nullptr;  // each base's absolute signal position
  unsigned* rpos = nullptr;  // the running maximum along each read of the column positions (the 64-bit sum of a
                             // column's n >= 1 votes' positions div n, 0 with no vote), 0 past the read's length
};
size_t assemble_work_bytes(int C, long long total, bool qual, bool mod, bool pos);
hipError_t launch_assemble_reads(const AsmArgs& a, hipStream_t s);
// the column quality's table, the doubles 10.0 ** (k / 10.0) for k < PHRED_LEVELS
#define PHRED_LEVELS 41
const double* phred_ratios();
// token weights: w[i] = min(65535, floor(65535 exp((double)lp) + 0.5)) with lp = logp[i][tokens[i]] (logp
// [n, V]) or tok_logp[i], exactly one of the two given; 0 for a token outside [0, V) or a non-finite lp
hipError_t launch_token_weights(const int* tokens, const float* logp, const float* tok_logp, int n, int V,
                                unsigned short* w, hipStream_t s);
// modification weights: mw[i] = 0 unless tokens[i] is canon or mod (two different ids in [0, V)); else, with
// d = (double)logp[i][canon] - (double)logp[i][mod], min(65535, floor(65535 / (1 + exp(d)) + 0.5)); a NaN d gives
// the hard call (65535 for mod, 0 for canon)
hipError_t launch_token_mod_weights(const int* tokens, const float* logp, int n, int V, int canon, int mod,
                                    unsigned short* mw, hipStream_t s);
// token positions: pos[b][s] (int32, [B, S]) = the running maximum over the steps of the rounded centroid of
// attention row s of chunk b (attn + b * ld_chunk + s * T, f32 probabilities) over t < min(span[b], T), in 24-bit
// fixed point and 64-bit integer sums (include/nanodec.h nd_token_positions has the rule); T <= TOKEN_POS_MAX_T
// keeps 2 M + Q inside 64 bits whatever the row holds
#define TOKEN_POS_MAX_T (1 << 19)
hipError_t launch_token_positions(const float* attn, long long ld_chunk, const int* span, int B, int S, int T,
                                  int* pos, hipStream_t s);
// global alignment of called reads to known sequences (align.hip, which states the rule): pair p is
// call[call_off[p] .. call_off[p+1]) against the same slice of truth; counts [P, 5] = {dist, n_match, n_sub, n_ins,
// n_del}, ops (nullable) one byte per call base, status [P] (bit 0: a side above ALIGN_MAX_LEN; bit 1: the pair's
// directions did not fit, cells understated); work holds align_work_bytes(P, cells) bytes, 8-byte aligned
#define ALIGN_MAX_LEN 8192
#define ALIGN_MAX_CELLS (1ll << 60)
long long align_work_bytes(int P, long long cells);
hipError_t launch_align_seqs(const unsigned char* call, const int* call_off, const unsigned char* truth,
                             const int* truth_off, int P, long long cells, int* counts, unsigned char* ops,
                             int* status, void* work, hipStream_t s);
// read mapping against a shared reference (locate.hip states the rule): segment p is call[call_off[p] ..
// call_off[p+1]); the index is the reference's 15-mers as (code, pos) sorted by code then pos; hit [P, 4] =
// {strand, w0, w1, votes}, status [P] (bit 0: unmapped), call_or the oriented bytes laid out like call
#define MAP_K 15
#define MAP_OCC_MAX 8
#define MAP_SEG 4096
#define MAP_BIN_SHIFT 9
#define MAP_PAD 1024
#define MAP_MIN_VOTES 8
#define MAP_REF_MAX (1 << 23)
hipError_t launch_locate_segs(const unsigned char* call, const int* call_off, int P, const unsigned* idx_code,
                              const unsigned* idx_pos, int idx_len, const int* rec_off, int R, int* hit, int* status,
                              unsigned char* call_or, hipStream_t s);
// the fit form of the alignment (align.hip): pair p is call[call_off[p] .. call_off[p+1]) against ref[hit[p][1] ..
// hit[p][2]) with free ends on the reference side; a pair whose status has bit 0 set on entry is skipped; span
// [P, 2] = the aligned reference interval in ref's coordinates; status bit 1: cells understated, bit 2: a side
// above ALIGN_MAX_LEN or a window outside [0, ref_len].  rpos (nullable: the form without positions) is one more
// output: rpos [call_off[P]] = the reference position of every oriented call base (the base matched or mismatched
// to; for an inserted base the one to its left), -1 for a pair that is not aligned
hipError_t launch_align_fit(const unsigned char* call, const int* call_off, const unsigned char* ref, int ref_len,
                            const int* hit, int P, long long cells, int* counts, int* span, unsigned char* ops,
                            int* status, int* rpos, void* work, hipStream_t s);
// consensus of the mapped reads (pileup.hip states the rule): pile [9, ref_len] u32, planes A, C, G, T, D, iA, iC,
// iG, iT; add piles the pairs of status 0 by their ops and rpos (one launch), call reads the pile into cons, ins
// (u8, 255 = none), cov and rec [R, 6] = {called, match, sub, del, ins, cov_sum}, which it zeroes itself
hipError_t launch_pileup_add(const unsigned char* call, const int* call_off, const unsigned char* ops, const int* rpos,
                             const int* status, int P, unsigned* pile, int ref_len, hipStream_t s);
hipError_t launch_pileup_call(const unsigned* pile, const unsigned char* ref, int ref_len, const int* rec_off, int R,
                              int min_cov, unsigned char* cons, unsigned char* ins, int* cov, long long* rec,
                              hipStream_t s);
// average self-attention (aan.hip): xn = LN_1(x), avg = (xn + step prev) / (step + 1)
// (prev from hist[anc[r][step-1]][step-1], avg stored at hist[r][step]), avg's
// row statistics (one partial); then q1 = sig(g_in) xn + sig(g_f) a + x (+ stats)
struct AanPrepArgs {
  const float* x = nullptr;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  float* hist = nullptr;
  const int* anc = nullptr;  // nullptr: identity
  int anc_ld = 0, step = 0, max_steps = 0;
  float* xn = nullptr;
  float* avg = nullptr;
  float* avg_part = nullptr;
  int R = 0;
};
hipError_t launch_aan_prep(const AanPrepArgs& a, hipStream_t s);
hipError_t launch_aan_gate(const float* g, const float* xn, const float* a, const float* x, float* out, float* part,
                           int R, hipStream_t s);
// random sampling (translate/translator.py:371-394): temperature, top-k
// (-1: the full distribution), and the draw's seed (device word, so one
// captured graph serves every seed); temp == 0 or topk == 1 is argmax
struct Sampling {
  float temp = 1.f;
  int topk = 1;
  const unsigned long long* seed = nullptr;
};
// One greedy head (search.hip / head.hpp greedy_head_row): LN_dec ->
// generator -> log_softmax -> argmax (or a sample) for a row, its token into
// tok / out_tokens[row][step], score, optional logp dump [R][S][V], and the
// next step's embedded input (ne).  Run by greedy_head_kernel, or by the
// layer-0 self-attention of the next step (SelfAttnArgs.head).
struct GreedyHead {
  const float* x = nullptr;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  const float* gw = nullptr;
  const float* gb = nullptr;
  int V = 0, S = 0, min_len = 0, eos = 0;
  int* tok = nullptr;
  int* out_tokens = nullptr;
  float* score = nullptr;
  float* logp_dump = nullptr;
  NextEmbed ne;
  Sampling smp;
};
hipError_t check_greedy_head(const GreedyHead& h);
// the standalone head of R rows: their token into column step of out_tokens
hipError_t launch_dec_greedy_head(const GreedyHead& h, int step, int R, hipStream_t s);

struct BeamState {
  float* cum;        // [C, beam] topk_log_probs
  int* seq[2];       // [C*beam, S] alive_seq (without BOS), double buffered
  int* anc[2];       // [C*beam, S] self-attn cache slot ancestry, double buffered
  int* tok;          // [C*beam] next decoder input
  int* done;         // [C]
  int* top_fin;      // [C]
  int* n_hyp;        // [C] hypotheses found so far
  float* hyp_score;  // [C, n_best]
  int* hyp_len;      // [C, n_best]
  int* hyp_tok;      // [C, n_best, S]
  int* n_alive;      // [1] chunks (classic: reference batches) not done
  int* steps_done;   // [1] decoder steps until the last chunk finished
  // classic onmt Beam (translate/translator.py:827-926): the reference batch
  // each chunk belongs to; a batch keeps advancing all of its beams until
  // every one of them is done
  int* group;        // [C] reference batch id
  int* grp_left;     // [C] chunks of the batch not done yet
  int* grp_done;     // [C] 0 while the batch is alive, else 1 + the step it finished in (its beams run that step, none after)
  int* steps_run;    // [C] advance() calls made on the chunk's beam (--fast: the step count when it was dropped)
  int* hyp_anc;      // [C, n_best, S] decoder row that ran each step of the hypothesis (its attention rows)
  // classic Beam: GNMTGlobalScorer state (onmt/translate/beam.py:181-243) and n-gram blocking (:100-119)
  float* cov[2];     // [C*beam, T] coverage = sum of the hypothesis' attention rows, double buffered
  float* pen;        // [C*beam] cov_penalty(coverage) of the live beams (score(), sort_finished)
  float* prev_pen;   // [C*beam] global_state["prev_penalty"] (stepwise penalty)
  int* blk[2];       // [C*beam] the hypothesis repeats an n-gram, double buffered
  const float* attn; // [C*beam][S][T] head-0 context attention probabilities, null when not captured
  const int* cut;    // [C] attention length of the chunk's beams (memory_lengths[j], translator.py:902-907)
  int T;             // attention row stride
};
// classic Beam options (translate/translator.py:113-173, onmt/translate/beam.py, penalties.py)
struct ClassicOpts {
  int lp_kind;     // length penalty: 0 none, 1 wu, 2 avg
  float alpha;
  float beta;
  int cov_kind;    // coverage penalty: 0 none, 1 wu, 2 summary
  int stepwise;    // -stepwise_penalty
  int ngram;       // -block_ngram_repeat (0: off)
  unsigned excl;   // -ignore_when_blocking token ids as a bit mask
};
// the output head's weights and input rows (host-only): LN_dec (ln_g, ln_b) -> generator (gw, gb) over V tokens
struct Generator {
  const float* x = nullptr;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  const float* gw = nullptr;
  const float* gb = nullptr;
  int V = 0;
};
// one search call: rows.C chunks of rows.rpc = beam_size rows (the tail's chunk list: the --fast beam only)
struct BeamCall {
  RowSet rows;
  int n_best = 1, S = 0, min_len = 0, eos = 0;
};
hipError_t launch_beam_init(const BeamState& st, int C, int beam, int bos, hipStream_t s);
// the --fast beam's length penalty of a step (translate/translator.py:718-720: ((5 + step + 1) / 6) ** alpha, a
// Python float the reference's division rounds to fp32): launch_beam_step's lenpen, for the engine and
// nd_op_beam_step alike
inline float fast_beam_lenpen(int step, float alpha) {
  return (float)std::pow((5.0 + (step + 1)) / 6.0, (double)alpha);
}
hipError_t launch_beam_step(const NextEmbed& ne, const Generator& g, const BeamState& st, const BeamCall& b, int step,
                            float lenpen, hipStream_t s);
hipError_t launch_beam_finish(const BeamState& st, int C, int n_best, int S, int* tokens, float* scores, int* lens,
                              hipStream_t s);
// classic Beam: length_penalty 0 none, 1 wu, 2 avg (onmt/translate/penalties.py)
hipError_t launch_beam_classic_init(const BeamState& st, const int* group, int C, int beam, int bos, hipStream_t s);
hipError_t launch_beam_classic_step(const NextEmbed& ne, const Generator& g, const BeamState& st, const BeamCall& b,
                                    int step, const ClassicOpts& o, hipStream_t s);
hipError_t launch_beam_classic_finish(const BeamState& st, int C, int beam, int n_best, int S, const ClassicOpts& o,
                                      int* tokens, float* scores, int* lens, hipStream_t s);
// per-step softmax of the captured head-0 scores of R rows (row r belongs to
// chunk r / rpc; keys t < span), in place at a[r * ld + t], zero for t >= span
hipError_t launch_attn_step_softmax(float* a, size_t ld, const int* span, int R, int rpc, int T, hipStream_t s);
// attention of each hypothesis along its ancestry: out[c][k][t][:] =
// attn[hyp_anc[c][k][t]][t][:] for t < hyp_len[c][k], zero after
hipError_t launch_beam_attn_gather(const BeamState& st, int C, int n_best, int S, int max_len, int T, float* out,
                                   hipStream_t s);

// ---- teacher-forced scoring (score.hip) ------------------------------------
// x[c*L + i][:] = emb[i == 0 ? bos : gold[c][i-1]] (* 16 + pe[i] with position encoding; the token clamped
// into [0, V)), row-major, and the row's statistics in one partial (part, ND_PART_LD slots per row)
hipError_t launch_tf_embed(const int* gold, int bos, int V, const float* emb, const float* pe, float* x, float* part,
                           int B, int L, hipStream_t s);
// fp32 attention of Lq query rows per chunk (row c*Lq + i of q, pitch ldq, head h at column 32 h) over the
// chunk's Lk key rows (row c*Lk + t of kv, pitch ldkv; K at column koff, V at voff): out [B*Lq, 256].
// causal: keys j <= i (Lq == Lk; mask unused).  Otherwise the context attention's mask over Lk keys.
// tap (context attention only; a causal launch with one is refused): head 0's masked scores before the
// softmax, tap[(c * Lq + i) * ld_tap + t] for i < Lq and every key t < Lk the chunk's workgroups walk (all
// t < min(span[c], Lk), the 32-key block around that edge included): the fp32 score, ND_MASK_FILL for a
// masked key, -inf for an absent one.  ld_tap >= Lk floats; columns at or past Lk are never written.  out
// is bit for bit what the launch without a tap writes; launch_attn_rows_softmax turns a dense tap
// (ld_tap == Lk) into probabilities.
struct TfAttnArgs {
  const float* q = nullptr;
  int ldq = 0;
  const float* kv = nullptr;
  int ldkv = 0, koff = 0, voff = 0;
  SrcMask mask;
  float* out = nullptr;
  int B = 0, Lq = 0, Lk = 0;
  bool causal = false;
  float* tap = nullptr;
  int ld_tap = 0;
};
hipError_t launch_tf_attention(const TfAttnArgs& a, hipStream_t s);
// per row c*L + i of g.x (row-major): LN_dec -> generator -> log_softmax; tok_logp[c][i] (nullable) =
// logp[gold[c][i]] for i < gold_len[c], else 0; score[c] = their sum in a fixed order; logp (nullable)
// [B, L, V] every row's log-probabilities.  L <= 512, V <= 32.
hipError_t launch_score_head(const Generator& g, const int* gold, const int* gold_len, int B, int L, float* score,
                             float* tok_logp, float* logp, hipStream_t s);
// K candidate slots per chunk, slot (c, k) empty when cand_len[c][k] <= 0: score_out[c][k] = score[c][k], -inf
// for an empty slot (score_out may be score); post[c][k] (nullable) = score - logsumexp over the chunk's
// non-empty slots, -inf for an empty one; best[c] (nullable) = the non-empty slot of the largest score, the
// lowest on a tie, -1 when all are empty.  One thread per chunk, slots in order: see cand_posterior_kernel.
hipError_t launch_cand_posterior(const float* score, const int* cand_len, int B, int K, float* score_out, float* post,
                                 int* best, hipStream_t s);

}  // namespace nd
