// Private to the host code of libnanodec_hip.so (engine.hip, model.hip, ops_api.hip): the context and
// model structs, the error helpers and the fluent GEMM launch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/nanodec.h"
#include "common.hpp"
#include "kernels.hpp"

// nd_last_error's text: one thread-local string for the whole library (defined in engine.hip)
extern thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail(ND_ERR_HIP, std::string(#expr) + " failed: " + hipGetErrorString(e_));      \
  } while (0)

#define LCHK(expr)                                                                    \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                      \
      return e_;                                                                      \
    }                                                                                 \
  } while (0)

struct Slot {
  float* dst = nullptr;
  std::vector<int64_t> shape;  // expected shape
  size_t numel = 0;
  bool loaded = false;
  bool required = true;
  int copy_rows = -1;  // >= 0: copy only the first copy_rows rows (pe table)
};

// n* = LayerNorm-folded copies (gamma into the weight columns, beta into the
// bias; derived at finalize): the GEMM prologue only normalises rows.
struct EncLayer {
  float *ln_g, *ln_b, *wqkv, *bqkv, *wo, *bo, *fln_g, *fln_b, *w1, *b1, *w2, *b2;
  float *nwqkv, *nbqkv, *nw1, *nb1;
  // P16H images of W1' (LN folded) and W2 for the fused FFN block (ffn.hip)
  uint16_t *w1h = nullptr, *w2h = nullptr;
  float w1s = 1.f, w2s = 1.f;
  // P16H image of Wo, folded into the FFN block's launch (ffn.hip WO)
  uint16_t* woh = nullptr;
  float wos = 1.f;
  // P16H image of the LN-folded W_qkv, folded into the previous layer's FFN launch (ffn.hip QK)
  uint16_t* qkvh = nullptr;
  float qkvs = 1.f;
};
struct DecLayer {
  float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *cwq, *cbq, *cwo, *cbo, *fln_g, *fln_b, *w1, *b1,
      *w2, *b2;
  float *nwqkv, *nbqkv, *ncwq, *ncbq, *nw1, *nb1;
  // P16-packed step weights (kernels.hpp launch_gemm_p16), derived at finalize
  float *pwqkv, *pwo, *pcwq, *pcwo, *pw1, *pw2;
  // memory-bank context attention (greedy): ctx K folded into the query
  // projection, ctx V into the output projection (derived at finalize, f64)
  float *pwqk, *bqk, *pwvo, *bvo;
  // average self-attention (onmt/modules/average_attn.py): average_layer FFN
  // (LN + 256 -> 256 -> 256) and gating Linear(512, 512); derived: LN-folded
  // P16 w_1, P16 w_2, the gate's xn / a column halves P16
  float *aln_g = nullptr, *aln_b = nullptr, *aw1 = nullptr, *ab1 = nullptr, *aw2 = nullptr, *ab2 = nullptr,
        *gw = nullptr, *gb = nullptr;
  float *naw1 = nullptr, *nab1 = nullptr, *paw1 = nullptr, *paw2 = nullptr, *pgwx = nullptr, *pgwa = nullptr;
};
struct NanoLayer {
  float *wih, *bih, *bhh, *whh, *bn_g, *bn_b, *bn_rm, *bn_rv;  // raw
  float *bsum, *bn_scale, *bn_shift;                             // derived at finalize
  int in;
};

// What a captured graph depends on.  Callers fill the fields by name; every field takes part in the order.
struct GraphKey {
  int mode = 0;  // 0 greedy / sampling, 1 --fast beam, 2 classic beam, 3 teacher-forced scoring (S = L)
  int B = 0, T = 0, S = 0, min_len = 0, beam = 1, n_best = 1;
  int K = 0;  // scoring: candidate slots per chunk (nd_score_candidates); 0 = nd_score_targets, no posterior
  int seg = 0;   // beam: first step of the segment, -1 = the prologue (encoder, memory, init)
  int logp = 0;  // greedy: per-step log-probabilities kept; scoring: bit 0 tok_logp, bit 1 logp kept
  float alpha = 0.f;
  int stamp = 0;  // kernel stamps on (set by run_graph from the ctx)
  // attention capture and the classic Beam's options
  int attn = 0, lenpen = 0, cov = 0, stepwise = 0, ngram = 0;
  unsigned excl = 0;
  float beta = 0.f;
  // random sampling (greedy path): top-k (1 = argmax) and temperature
  int topk = 1;
  float temp = 0.f;
  int exact = 0;  // exact fp32 products (set by run_graph from the ctx)
  int bank_nt = 0;  // memory bank streamed non-temporally (set by run_graph from the ctx)
  int bank_grid = 0;  // the bank kernel's workgroup cap (set by run_graph from the ctx)
  int splitk = 0;     // long-K step GEMMs split over workgroups (set by run_graph from the ctx)
  int tail = 0;   // --fast beam tail segments (nd_ctx.beam_tail)
  auto tie() const {
    return std::tie(mode, B, T, S, K, min_len, beam, n_best, seg, logp, alpha, stamp, attn, lenpen, cov, stepwise, ngram,
                    excl, beta, topk, temp, exact, tail, bank_nt, bank_grid, splitk);
  }
  bool operator<(const GraphKey& o) const { return tie() < o.tie(); }
};

// Everything nd_load_weight and nd_finalize produce and calls only read: the weight pointers and every image
// derived from them.  nd_share_weights hands a pooled lane the owner's Model in one assignment, so a field added
// here is shared without further code; a workspace or a per-call flag does not belong here.
struct Model {
  float *enc_lin_w = nullptr, *enc_lin_b = nullptr, *enc_ln_g = nullptr, *enc_ln_b = nullptr;
  // the memory bank's LayerNorm affine divided by its per-dimension power-of-two
  // scales (derive_bank_dim_scales; transformer encoder), and the scales
  float *bank_ln_g = nullptr, *bank_ln_b = nullptr;
  std::vector<float> bank_dim_scale;
  // encoder layer 0's QKV in the rank-2 form (kernels.hpp EmbedQkv): a | c on
  // the device, the three means and s0 on the host in eq (the kernel argument);
  // set at finalize (nd::prepare_embed_qkv)
  float* eq_ac = nullptr;
  double* eq_scal = nullptr;
  nd::EmbedQkv eq;
  // layer 0's attention in the same closed form: per head the 6 coefficients
  // of alpha_t, beta_t (launch_enc_attention_rank2), on the device
  float* eq_coef = nullptr;
  std::vector<EncLayer> enc;
  std::vector<NanoLayer> nano;
  float* nano_W = nullptr;
  std::vector<DecLayer> dec;
  float *ctxkv_w = nullptr, *ctxkv_b = nullptr, *nctxkv_w = nullptr, *nctxkv_b = nullptr;
  float *emb = nullptr, *pe = nullptr, *dec_ln_g = nullptr, *dec_ln_b = nullptr, *gen_w = nullptr, *gen_b = nullptr;
  // split-fp16 images of the row-major GEMM weights (gemm.hip, H3), keyed by
  // the fp32 weight they were made from (built at finalize)
  std::map<const float*, std::pair<uint16_t*, float>> split;
  // row-major split images of the P16 step weights (large-M route), keyed by the P16 weight
  std::map<const float*, std::pair<uint16_t*, float>> split_rm;
  // decoder layer 0's QKV table (kernels.hpp QkvRows; scaled-dot decoders): row step * V + token holds
  // q | k | v of that input, [round16(qtab_steps * V), 768] row-major, for every step a context may run
  // (qtab_steps = the owner's max_steps; a call of fewer steps reads a prefix).  It depends on the weights
  // alone, so nd_finalize builds it once in each product mode a call can run in: [0] through the split-fp16
  // step GEMM, [1] in exact fp32 (nd_set_exact_fp32 flips between them at run time)
  float* qtab[2] = {nullptr, nullptr};
  int qtab_steps = 0;
  // the table's input rows and their statistics: used while nd_finalize builds it, kept for the next nd_finalize
  float *qtab_x = nullptr, *qtab_part = nullptr;
};

struct nd_ctx {
  nd_config cfg{};
  int D = ND_D, F = 2048, V = 8, H = 128;
  Model m;  // its own after nd_finalize, or another context's (nd_share_weights)
  // load-time bookkeeping of the context that owns the weights
  std::map<std::string, Slot> slots;
  std::vector<void*> allocs;
  bool finalized = false;
  bool shares = false;  // reads another context's weights (nd_share_weights)
  bool use_graphs = true;
  int ctx_path = 0;  // 0: memory-bank form for greedy, K/V form for beam; 1: always K/V
  bool kstamp_on = false;                 // stamp every context-attention launch (bench roofline)
  unsigned long long* kstamp = nullptr;   // [dec_layers * max_steps][2] (start, end) wall-clock ticks
  bool timing = false;
  float t_enc = 0.f, t_dec = 0.f;
  // exact fp32: plain fp32-MFMA kernels everywhere (no split-fp16 products); nd_set_exact_fp32
  bool exact = false;
  // split-fp16 range guard word (common.hpp flag_overflow), read and cleared
  // per call by nd_take_overflow
  int* ovf = nullptr;
  // stream the memory bank with non-temporal loads (nd_set_bank_policy): an
  // EnginePool lane whose bank should not displace another lane's from the
  // Infinity Cache
  bool bank_nt = false;
  // workgroups of the bank kernel at most (nd_set_bank_grid; 0 = one per chunk)
  int bank_grid = 0;
  // the K = 2048 step GEMMs split over workgroups (gemm_p16k_kernel, nd_set_gemm_splitk).  Off by default:
  // a lone call is faster on the one-workgroup-per-tile long-K kernel; EnginePool lanes (several calls in
  // flight) turn it on ("Decoder GEMMs at 256 rows")
  bool splitk = false;

  // per-dimension power-of-two rebalancing of the decoder attentions' key / query and value / output
  // projections (rebalance_attention): for a weight buffer, the scale of each of its rows (or columns), which
  // nd_load_weight applies to a tensor loaded into it later so the set stays consistent
  struct Rescale {
    std::vector<float> s;
    bool cols = false;
  };
  std::map<const float*, Rescale> rescale;
  bool rebalanced = false;

  // per-call state, set by the translate_* drivers while their graphs are enqueued (CallFlags)
  bool attn_on = false;    // the call captures the attention
  bool beam_tail = false;  // --fast beam: few chunks alive (seen at a segment poll): the decoder GEMMs stay on
                           // the small-M P16 kernels (GraphKey.tail)

  // workspaces
  float* sig = nullptr;
  int *len = nullptr, *span = nullptr;
  float *x = nullptr, *y = nullptr, *att = nullptr, *big = nullptr, *ctxkv = nullptr;
  float* mem_p = nullptr;                 // memory bank [B * T, 256] row-major (LN'd encoder output)
  const float* mem = nullptr;             // the bank the decoder reads: mem_p, or x (NanoEncoder)
  bool bank_d8 = false;                   // mem_p holds the 24-bit digit bank (dec_bank_d8_kernel; bank8.hip)
  bool ctx_q24 = false;                   // beam rows read the 24-bit context K/V image (ctxq), not fp32 ctxkv
  int* clist = nullptr;                   // --fast beam tail: the alive chunks (launch_alive_list), ceil(B/16)
  float* ctx_part = nullptr;              // ... and the split context attention's partial states
  uint8_t* ctxq = nullptr;                // [layers][B * T][CTXQ_ROW] (attention.hip ctx_pack_q24_kernel)
  float* bank_ks = nullptr;               // digit bank: per-row scales 2^e_t [B * 512]
  int* bank_em = nullptr;                 // digit bank: per-chunk max e_t (biased) [B]
  int last_bank_form = 0;                 // nd_bank_form
  float *dqk = nullptr, *dU = nullptr;    // [R, 8*256] P16 (memory-bank path)
  float* sk_slab = nullptr;               // split-K P16 GEMMs: fp32 partial slabs (gemm_p16k_kernel)
  int* sk_cnt = nullptr;                  // ... and their per-tile tickets (zeroed per call)
  int sk_tiles = 0;                       // 32 x 32 tiles the slab serves
  float* dffn_slab = nullptr;             // beam rows' split fused FFN (ffn.hip DecFfn): partial slabs
  int* dffn_cnt = nullptr;                // ... and per-row-block tickets (zeroed per call)
  int dffn_rb = 0;                        // 128-row blocks they serve
  // average self-attention step buffers (P16): xn, avg (+ its row stats), the
  // average_layer hidden, a = FFN(avg), the gate pre-activations [R, 512]
  float *axn = nullptr, *aavg = nullptr, *aavg_part = nullptr, *ah = nullptr, *aa = nullptr, *ag = nullptr;
  float *nano_xp = nullptr, *nano_h = nullptr;
  float *x_part = nullptr, *y_part = nullptr, *dx_part = nullptr, *dq1_part = nullptr, *dmid_part = nullptr;
  int x_pn = 1;
  float *dx = nullptr, *dq1 = nullptr, *dmid = nullptr, *dcq = nullptr, *datt = nullptr, *dqkv = nullptr,
        *dhid = nullptr, *cache = nullptr;
  int *tok = nullptr, *gtok = nullptr;
  // each row's token of the step: its row of the layer-0 QKV table (Model.qtab)
  int* rtok = nullptr;
  float *gscore = nullptr, *glogp = nullptr;
  nd::BeamState bs{};
  int* steps_done = nullptr;
  int* group_in = nullptr;  // classic Beam: staged reference-batch ids
  int* cut_in = nullptr;    // classic Beam: staged attention lengths (coverage penalties)
  unsigned long long* seed_dev = nullptr;  // random sampling: the call's seed (read by the captured graph)
  // -attn_debug / coverage: [decoder rows][max_steps][max_src_len] head-0 context scores -> probabilities
  float* attn_raw = nullptr;
  int* h_alive = nullptr;  // pinned
  // teacher-forced scoring (nd_score_targets), made on first use: the [max_batch * max_steps, .] row-major
  // decoder rows x / q1 / mid / cq / att with their row statistics, q | k | v and the FFN hidden (tf_big: the
  // encoder's `big` when max_steps <= max_src_len, the encoder being done with it), the staged gold rows
  // and the results (tf_post / tf_best: nd_score_candidates' per-slot posterior and per-chunk best)
  float *tf_x = nullptr, *tf_q1 = nullptr, *tf_mid = nullptr, *tf_cq = nullptr, *tf_att = nullptr, *tf_big = nullptr;
  float *tf_x_part = nullptr, *tf_q1_part = nullptr, *tf_mid_part = nullptr;
  int *tf_gold = nullptr, *tf_gold_len = nullptr;
  float *tf_score = nullptr, *tf_tok_logp = nullptr, *tf_logp = nullptr, *tf_post = nullptr;
  int* tf_best = nullptr;

  hipStream_t es = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;
  std::map<GraphKey, hipGraphExec_t> graphs;
};

// the context's weight registry (model.hip); the graph cache (engine.hip): every captured graph read the
// weights or the setting that just changed
int build_registry(nd_ctx* c);
void drop_graphs(nd_ctx* c);

template <typename T>
inline hipError_t dalloc(nd_ctx* c, T** p, size_t n) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, n * sizeof(T) + 256);
  if (e != hipSuccess) return e;
  e = hipMemset(q, 0, n * sizeof(T) + 256);
  c->allocs.push_back(q);
  *p = reinterpret_cast<T*>(q);
  return e;
}

// Fluent GEMM launch: G(...).ln(...).res(...).stats(...).run(s, &part_n)
struct G {
  nd::GemmArgs a;
  G(const float* A, int lda, const float* W, int N, int K, const float* bias, float* C, int ldc, int M) {
    a.A = A; a.lda = lda; a.W = W; a.ldw = K; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  }
  // LayerNorm prologue (affine already folded into W / bias)
  G& ln(const float* part, int pn) {
    a.norm = true; a.part_in = part; a.part_n_in = pn;
    return *this;
  }
  G& relu() { a.relu = true; return *this; }
  // use the weight's split-fp16 image when finalize made one
  G& h3(const nd_ctx* c) {
    if (c->exact) return *this;  // fp32 weights only: the fp32-MFMA kernels
    auto it = c->m.split.find(a.W);
    if (it != c->m.split.end()) {
      a.Wh = it->second.first;
      a.wscale = it->second.second;
      a.ovf = c->ovf;
    }
    auto jt = c->m.split_rm.find(a.W);
    if (jt != c->m.split_rm.end()) {
      a.Wh_rm = jt->second.first;
      a.wscale_rm = jt->second.second;
    }
    return *this;
  }
  G& res(const float* R, int ldr) { a.R = R; a.ldr = ldr; return *this; }
  G& stats(float* part) { a.part_out = part; return *this; }
  G& skip(const int* done, int rpc) { a.skip = done; a.skip_rpc = rpc; return *this; }
  G& small_m(bool on) { a.prefer_p16 = on ? 1 : 0; return *this; }
  G& c_rowmajor(bool on) { a.c_rm = on ? 1 : 0; return *this; }  // P16 GEMMs: C row-major
  G& q24(uint8_t* img, size_t plane) { a.q24 = img; a.q24_plane = plane; return *this; }  // the 24-bit image, not C
  // long-K P16 products may split over workgroups (gemm_p16k_kernel) into the context's slab
  G& splitk(const nd_ctx* c) {
    if (!c->splitk) return *this;
    a.sk_slab = c->sk_slab;
    a.sk_cnt = c->sk_cnt;
    a.sk_tiles = c->sk_tiles;
    return *this;
  }
  bool packed = false;
  G& p16() { packed = true; return *this; }  // decoder-step operands in the P16 layout
  hipError_t run(hipStream_t s, int* pn_out = nullptr) {
    hipError_t e = packed ? nd::launch_gemm_p16(a, s) : nd::launch_gemm(a, s);
    if (pn_out) *pn_out = a.part_n_out;
    return e;
  }
};
