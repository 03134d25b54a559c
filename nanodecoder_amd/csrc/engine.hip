// libnanodec_hip.so — engine context, launch sequences, hipGraph capture and
// the context calls of the C-ABI of include/nanodec.h (the model side is
// model.hip, the op-level entry points ops_api.hip).
//
// One nd_ctx per device.  It owns:
//   * the packed fp32 weights (QKV of each attention fused into one [768,256]
//     matrix; the three decoder layers' context K/V projections fused into one
//     [3*512, 256] matrix so the memory bank is projected by ONE GEMM),
//   * encoder/decoder workspaces sized for (max_batch, max_src_len,
//     max_steps, max_beam),
//   * instantiated hipGraphs of whole translate calls, keyed by shape.
#include "engine.hpp"

thread_local std::string g_err;

// --------------------------------------------------------------- workspaces
static int alloc_ctx_kv(nd_ctx* c) {
  if (c->ctxkv) return ND_OK;
  const auto& cfg = c->cfg;
  const size_t B = cfg.max_batch, T = cfg.max_src_len, D = c->D, Ld = cfg.dec_layers;
  hipError_t e;
#define WSK(ptr, n)                                         \
  if ((e = dalloc(c, &(ptr), (size_t)(n))) != hipSuccess) \
    return fail(ND_ERR_HIP, std::string("hipMalloc workspace " #ptr ": ") + hipGetErrorString(e));
  WSK(c->ctxkv, B * T * Ld * 2 * D);
  float* q = nullptr;
  WSK(q, B * T * Ld * (CTXQ_ROW / 4));
  c->ctxq = reinterpret_cast<uint8_t*>(q);
  float* l = nullptr;
  WSK(l, B);
  c->clist = reinterpret_cast<int*>(l);
  // ceil(B/16) listed chunks x up to 32 splits x rows x {num[256], max[8], den[8]}
  WSK(c->ctx_part, (B + 15) / 16 * 32 * std::max(1, cfg.max_beam) * (D + 16));
  {
    // the beam's split fused FFN: up to 8 splits per 128-row block
    const int R = (int)((B * (size_t)std::max(1, cfg.max_beam) + 15) / 16 * 16);
    c->dffn_rb = (R + 127) / 128;
    WSK(c->dffn_slab, nd::dec_ffn_slab_floats(R, 8));
    float* t = nullptr;
    WSK(t, (size_t)(c->dffn_rb + 3) / 4 * 4);
    c->dffn_cnt = reinterpret_cast<int*>(t);
    if ((e = hipMemset(c->dffn_cnt, 0, (size_t)(c->dffn_rb + 3) / 4 * 16)) != hipSuccess)
      return fail(ND_ERR_HIP, std::string("hipMemset FFN tickets: ") + hipGetErrorString(e));
  }
#undef WSK
  return ND_OK;
}

static int alloc_workspaces(nd_ctx* c) {
  const auto& cfg = c->cfg;
  const size_t B = cfg.max_batch, T = cfg.max_src_len, S = cfg.max_steps;
  // decoder rows, padded to whole 16-row P16 blocks
  const size_t R = (B * (size_t)std::max(1, cfg.max_beam) + 15) / 16 * 16;
  const size_t D = c->D, F = c->F, Ld = cfg.dec_layers;
  hipError_t e;
#define WS(ptr, n)                                          \
  if ((e = dalloc(c, &(ptr), (size_t)(n))) != hipSuccess) \
    return fail(ND_ERR_HIP, std::string("hipMalloc workspace " #ptr ": ") + hipGetErrorString(e));
  WS(c->sig, B * T);
  WS(c->len, B);
  WS(c->span, B);
  WS(c->x, B * T * D);
  WS(c->y, B * T * D);
  WS(c->att, B * T * D);
  WS(c->big, B * T * std::max(F, 3 * D));
  // the per-layer context K/V (fp32 and the 24-bit image) and the beam tail's buffers: beam-capable
  // contexts only (a greedy context allocates them on nd_set_ctx_path(1)); ADVICE r04: 1.4 GB per
  // greedy lane at B = 256
  if (cfg.max_beam > 1) {
    const int rc = alloc_ctx_kv(c);
    if (rc != ND_OK) return rc;
  }
  {
    // split-K P16 GEMMs (K = 2048 / 1024 at 128 < R <= 1024): 32 x 32 tiles x 4 slices x 4 KB
    const int tiles = (int)std::min<size_t>((R + 31) / 32, 32) * (int)(D / 32);
    WS(c->sk_slab, (size_t)tiles * 4 * 1024);
    float* t = nullptr;
    WS(t, (size_t)(tiles + 3) / 4 * 4);
    c->sk_cnt = reinterpret_cast<int*>(t);
    c->sk_tiles = tiles;
    if ((e = hipMemset(c->sk_cnt, 0, (size_t)(tiles + 3) / 4 * 16)) != hipSuccess)
      return fail(ND_ERR_HIP, std::string("hipMemset split-K tickets: ") + hipGetErrorString(e));
  }
  // the fp32 bank [B * T, 256], or the digit bank: 512 rows per chunk whatever T is (B * 512 * 256 * 3 bytes)
  WS(c->mem_p, std::max(B * T * D, B * 512 * ND_D * 3 / 4));
  WS(c->bank_ks, B * 512);
  {
    float* em = nullptr;
    WS(em, B);
    c->bank_em = reinterpret_cast<int*>(em);
  }
  WS(c->x_part, B * T * ND_PART_LD * 2);
  WS(c->y_part, B * T * ND_PART_LD * 2);
  WS(c->dx_part, R * ND_PART_LD * 2);
  WS(c->dq1_part, R * ND_PART_LD * 2);
  WS(c->dmid_part, R * ND_PART_LD * 2);
  if (cfg.encoder_type == ND_ENC_NANO) {
    WS(c->nano_xp, B * T * 8 * (size_t)c->H);
    WS(c->nano_h, B * T * 2 * (size_t)c->H);
  }
  WS(c->dx, R * D);
  WS(c->dq1, R * D);
  WS(c->dmid, R * D);
  WS(c->dcq, R * D);
  WS(c->datt, R * D);
  WS(c->dqkv, R * 3 * D);
  WS(c->dhid, R * F);
  WS(c->dqk, R * ND_H * D);
  WS(c->dU, R * ND_H * D);
  if (cfg.self_attn_type == ND_SELF_AVERAGE) {
    WS(c->axn, R * D);
    WS(c->aavg, R * D);
    WS(c->aavg_part, R * ND_PART_LD * 2);
    WS(c->ah, R * D);
    WS(c->aa, R * D);
    WS(c->ag, R * 2 * D);
  }
  WS(c->cache, Ld * R * S * 2 * D);
  WS(c->tok, R);
  if (cfg.self_attn_type != ND_SELF_AVERAGE) {
    WS(c->rtok, R);
  }
  WS(c->gtok, B * S);
  WS(c->gscore, B);
  WS(c->glogp, B * S * (size_t)c->V);
  WS(c->bs.cum, R);
  WS(c->bs.seq[0], R * S);
  WS(c->bs.seq[1], R * S);
  WS(c->bs.anc[0], R * S);
  WS(c->bs.anc[1], R * S);
  c->bs.tok = c->tok;
  WS(c->bs.done, B);
  WS(c->bs.top_fin, B);
  WS(c->bs.n_hyp, B);
  const size_t NB = (size_t)std::max(1, cfg.max_beam);
  WS(c->bs.hyp_score, B * NB);
  WS(c->bs.hyp_len, B * NB);
  WS(c->bs.hyp_tok, B * NB * S);
  WS(c->bs.n_alive, 4);
  WS(c->steps_done, 4);
  c->bs.steps_done = c->steps_done;
  WS(c->bs.group, B);
  WS(c->bs.grp_left, B);
  WS(c->bs.grp_done, B);
  WS(c->bs.steps_run, B);
  WS(c->bs.hyp_anc, B * NB * S);
  WS(c->bs.cov[0], R * T);
  WS(c->bs.cov[1], R * T);
  WS(c->bs.pen, R);
  WS(c->bs.prev_pen, R);
  WS(c->bs.blk[0], R);
  WS(c->bs.blk[1], R);
  c->bs.T = (int)T;
  WS(c->group_in, B);
  WS(c->cut_in, B);
  WS(c->seed_dev, 2);
  WS(c->kstamp, Ld * S * 2);
  WS(c->ovf, 4);
#undef WS
  if ((e = hipHostMalloc((void**)&c->h_alive, 16, hipHostMallocDefault)) != hipSuccess)
    return fail(ND_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  return ND_OK;
}

// ------------------------------------------------------------ launch sequences
// Encoder forward (transformer): x <- memory before the final LayerNorm (its
// row statistics in x_part); the final LN is the ctx-K/V GEMM's prologue.
//
// Layer 0 runs in the rank-2 closed form (EmbedQkv, launch_enc_attention_rank2):
// no q | k | v rows at all for layer 0 (encoder 3.65 -> 3.40 ms per 256-chunk
// call), evaluated about the sample s0 where the row variance is least
// (m.eq, prepared at finalize), which keeps it within fp32 rounding of the
// materialised layer however w' and b' lie.  Its LDS is exactly 64 KB: the round-3 layout (67,584 B, wave 7's
// E[y] / E[r] rows read and written past byte 65,536 by ds_read2 / ds_write2)
// returned wrong chunks whenever another engine's decoder GEMMs shared the CU;
// every layout whose accesses stay below 65,536 is clean (tools/r2_lds.sh,
// DESIGN.md section 5).
//
// On the split-fp16 path a layer's Wo + residual, LN and FFN are one launch
// (ffn.hip; y never written, the layer's rows updated in place) that also
// projects the next layer's q | k | v from its registers.  Exact fp32, or a
// d_ff the block does not take (no w1h image), keeps the GEMMs; same arithmetic.
static hipError_t enqueue_encode_transformer(nd_ctx* c, int B, int T, hipStream_t s) {
  const Model& m = c->m;
  const int M = B * T, D = c->D, F = c->F;
  LCHK(nd::launch_enc_embed(c->sig, m.enc_lin_w, m.enc_lin_b, c->x, c->x_part, B, T, s));
  int pnx = 1, pny = 0;
  bool qkv_done = false;  // this layer's q | k | v already in c->big
  for (size_t li = 0; li < m.enc.size(); ++li) {
    const EncLayer& L = m.enc[li];
    // encoder/transformer.py:36-54
    if (li == 0) {
      LCHK(nd::launch_enc_attention_rank2({.signal = c->sig, .span = c->span, .eq = m.eq, .coef = m.eq_coef,
                                           .out = c->att}, B, T, s));
    } else {
      if (!qkv_done) LCHK(G(c->x, D, L.nwqkv, 3 * D, D, L.nbqkv, c->big, 3 * D, M).h3(c).ln(c->x_part, pnx).run(s));
      LCHK(nd::launch_enc_attention({.qkv = c->big, .mask = {c->sig, c->span}, .out = c->att, .B = B, .T = T,
                                     .exact = c->exact, .ovf = c->ovf}, s));
    }
    qkv_done = false;
    if (!c->exact && L.w1h) {  // the fused block (nd_finalize makes w1h, w2h, woh and qkvh together)
      nd::EncQkv qk;  // the next layer's q | k | v, when there is one
      if (li + 1 < m.enc.size()) {
        const EncLayer& N = m.enc[li + 1];
        qk = {.wh = N.qkvh, .ws = N.qkvs, .bias = N.nbqkv, .out = c->big};
        qkv_done = qk.wh != nullptr;
      }
      LCHK(nd::launch_enc_ffn({.y = c->x, .w1h = L.w1h, .w1s = L.w1s, .b1 = L.nb1, .w2h = L.w2h, .w2s = L.w2s,
                               .b2 = L.b2, .x = c->x, .xpart = c->x_part, .M = M, .F = F, .ovf = c->ovf},
                              {.att = c->att, .woh = L.woh, .wos = L.wos, .bo = L.bo}, qk, s));
      pnx = 1;
      continue;
    }
    LCHK(G(c->att, D, L.wo, D, D, L.bo, c->y, D, M).h3(c).res(c->x, D).stats(c->y_part).run(s, &pny));
    LCHK(G(c->y, D, L.nw1, F, D, L.nb1, c->big, F, M).h3(c).ln(c->y_part, pny).relu().run(s));
    LCHK(G(c->big, F, L.w2, D, F, L.b2, c->x, D, M).h3(c).res(c->y, D).stats(c->x_part).run(s, &pnx));
  }
  c->x_pn = pnx;
  return hipSuccess;
}

// NanoEncoder (encoder/nano_encoder.py:79-124): 3x BiLSTM; layers 0-1 emit
// BatchNorm(h) for the next layer, layer 2 emits raw h (zeros at padded
// steps, as pad_packed_sequence does); memory = h W^T -> c->x.
static hipError_t enqueue_encode_nano(nd_ctx* c, int B, int T, hipStream_t s) {
  const Model& m = c->m;
  const int M = B * T, D = c->D, Lz = (int)m.nano.size();
  float* bufs[2] = {c->y, c->att};
  for (int l = 0; l < Lz; ++l) {
    const NanoLayer& L = m.nano[l];
    float* out = bufs[l & 1];
    const bool last = l == Lz - 1;
    if (l > 0)
      LCHK(G(bufs[(l - 1) & 1], 2 * c->H, L.wih, 8 * c->H, 2 * c->H, L.bsum, c->nano_xp, 8 * c->H, M).h3(c).run(s));
    if (last) LCHK(hipMemsetAsync(out, 0, (size_t)M * 2 * c->H * sizeof(float), s));
    LCHK(nd::launch_lstm_layer({.xp = c->nano_xp, .signal = c->sig, .wih0 = L.wih, .bsum = L.bsum, .whh = L.whh,
                                .len = c->len, .B = B, .T = T, .out = out, .bn_scale = last ? nullptr : L.bn_scale,
                                .bn_shift = last ? nullptr : L.bn_shift, .layer0 = l == 0, .exact = c->exact}, s));
  }
  return G(bufs[(Lz - 1) & 1], 2 * c->H, m.nano_W, D, 2 * c->H, nullptr, c->x, D, M).h3(c).run(s);
}

static hipError_t enqueue_encode(nd_ctx* c, int B, int T, hipStream_t s) {
  // every call starts with the split-K tickets at zero (a memset node in the call's graph): each tile's last
  // arriver resets its own, this repairs a ticket left by an aborted call (cdna_hip_programming.md §6,
  // Guideline 16 "Re-initialise every call")
  if (c->sk_cnt) LCHK(hipMemsetAsync(c->sk_cnt, 0, (size_t)(c->sk_tiles + 3) / 4 * 16, s));
  if (c->dffn_cnt) LCHK(hipMemsetAsync(c->dffn_cnt, 0, (size_t)(c->dffn_rb + 3) / 4 * 16, s));
  if (c->cfg.encoder_type == ND_ENC_TRANSFORMER) return enqueue_encode_transformer(c, B, T, s);
  return enqueue_encode_nano(c, B, T, s);
}

// q24: the GEMM's epilogue writes the 24-bit image (ctxq) instead of fp32 K/V
static hipError_t enqueue_ctxkv(nd_ctx* c, int B, int T, hipStream_t s, bool q24) {
  const int M = B * T, D = c->D, N = (int)c->m.dec.size() * 2 * D;
  uint8_t* img = q24 ? c->ctxq : nullptr;
  const size_t plane = (size_t)M * CTXQ_ROW;  // one layer's keys of the call (enqueue_dec_step reads the same)
  if (c->cfg.encoder_type == ND_ENC_TRANSFORMER)
    return G(c->x, D, c->m.nctxkv_w, N, D, c->m.nctxkv_b, c->ctxkv, N, M).h3(c).ln(c->x_part, c->x_pn).q24(img, plane).run(s);
  return G(c->x, D, c->m.ctxkv_w, N, D, c->m.ctxkv_b, c->ctxkv, N, M).h3(c).q24(img, plane).run(s);
}

// Layer 0 of a scaled-dot decoder reads q | k | v from the model's table
// QKV0[step][token] (kernels.hpp, QkvRows; Model.qtab, built by nd_finalize in
// the call's product mode) instead of running its QKV GEMM every step.
// Average-attention decoders have no table and keep the per-step GEMM.  With
// the table, the greedy head is fused into the next step's layer-0
// self-attention, and a greedy row's layer-0 history is read from the table
// too (QkvRows.hist): greedy calls do not touch layer 0's region of the cache.
static const float* qkv_table(const nd_ctx* c) { return c->m.qtab[c->exact ? 1 : 0]; }
static bool head_fused(const nd_ctx* c) { return qkv_table(c) && c->V <= 8; }  // SELF_TABV

static nd::NextEmbed next_embed(nd_ctx* c) {
  nd::NextEmbed ne;
  ne.emb = c->m.emb;
  ne.pe = c->cfg.position_encoding ? c->m.pe : nullptr;
  ne.x = c->dx;
  ne.part = c->dx_part;
  ne.tok = qkv_table(c) ? c->rtok : nullptr;
  return ne;
}

// Step-0 decoder input (later steps' inputs are written by the search
// kernel that picks their token).
static hipError_t enqueue_first_embed(nd_ctx* c, int R, hipStream_t s) {
  return nd::launch_dec_embed(c->tok, c->m.emb, c->cfg.position_encoding ? c->m.pe : nullptr, 0, c->dx, c->dx_part, R, s);
}

// One decoder step for R = C*rpc rows: dx (embedded input, row stats in
// dx_part) -> dx (pre final LN).
// greedy rows always take the memory-bank form (ctx path 0); beam rows read
// the per-layer context K/V
static bool use_memory_bank(nd_ctx* c, int rpc) { return c->ctx_path == 0 && rpc == 1; }

// The A/B switches (environment variables, read once per process): each name and default is written here
// and nowhere else.  The launch sequences read them through switch_value; nd_switches reports the ones set
// to something else.
enum Switch { SW_CTX_SPLIT, SW_DEC_FFN, SW_N };
static const struct {
  const char* name;
  int def;
} kSwitches[SW_N] = {{"ND_CTX_SPLIT", 16}, {"ND_DEC_FFN", 1}};

static int switch_value(Switch sw) {
  static const std::vector<int> v = [] {
    std::vector<int> r;
    for (const auto& k : kSwitches) {
      const char* e = getenv(k.name);
      r.push_back(e ? atoi(e) : k.def);
    }
    return r;
  }();
  return v[sw];
}

// --fast beam tail: the context attention over a chunk's keys in this many workgroups (one per CU: a lone
// chunk's 512 keys are latency-bound on one workgroup, ~150 us); ND_CTX_SPLIT=1 keeps one per chunk
static int ctx_split() { return std::min(32, std::max(1, switch_value(SW_CTX_SPLIT))); }

// The decoder's view of the encoder output: a pure function of (ctx path,
// exact, T, rpc, encoder type).  Set on the host before every call's graphs
// run or are captured: a replayed encoder graph does not re-enter
// enqueue_memory, but the step graphs captured after it read these fields.
// Beam rows read the context K/V in 24-bit fixed point (ctxq; 0.78x the bytes of
// the HBM-bound context attention); exact fp32 keeps fp32 K/V.
static void set_memory_view(nd_ctx* c, int T, int rpc) {
  c->bank_d8 = false;
  c->mem = nullptr;
  c->last_bank_form = 0;
  c->ctx_q24 = !use_memory_bank(c, rpc) && !c->exact;
  if (c->ctx_q24) c->last_bank_form = 3;
  if (!use_memory_bank(c, rpc)) return;
  const bool tf = c->cfg.encoder_type == ND_ENC_TRANSFORMER;
  // 512-sample chunks: the 24-bit digit bank (LN'd for the transformer, the
  // NanoEncoder's output as it stands)
  c->bank_d8 = !c->exact && nd::bank_eligible(T, c->cfg.max_src_len);
  c->mem = (c->bank_d8 || tf) ? c->mem_p : c->x;  // the NanoEncoder's fp32 output is the bank as it stands
  c->last_bank_form = c->bank_d8 ? 2 : 0;
}

// The beam's decoder FFN as one fused launch (ffn.hip launch_dec_ffn) at
// R >= 1024 rows outside the tail: d_ff split so that about 160 workgroups
// (one per CU, 128 KB of LDS each) run at once, at most 8 splits per row
// block (the last arriver reads the others' 128 KB partials).  Measured at
// R = 5120 (40 row blocks, configs[3], same box, two reps each): 3 / 4 / 5 /
// 6 / 8 splits = 70.3-71.0 / 70.1-70.6 / 71.8-72.0 / 71.0-71.2 / 71.4-72.0 ms
// per pooled call (one call: 89.5 / 88.2 / 87.2 / 87.0 / 91.1 ms); the two
// GEMMs 74.0 / 92.6.  0: the two GEMMs (greedy rows, the tail, exact fp32,
// no split images).
// ND_DEC_FFN=0 keeps the GEMMs, ND_DEC_FFN=n > 1 forces n splits (A/B).
static int dec_ffn_splits(const nd_ctx* c, int R) {
  const int knob = switch_value(SW_DEC_FFN);
  if (knob == 0 || c->exact || c->beam_tail || !c->dffn_slab || R < 1024 || R % 16) return 0;
  const int F = c->F;
  const DecLayer& L = c->m.dec[0];
  if (F % 32 || F > 2048 || !c->m.split.count(L.pw1) || !c->m.split.count(L.pw2)) return 0;
  const int rb = (R + 127) / 128;
  if (rb > c->dffn_rb) return 0;
  if (knob > 1) return std::min({knob, 8, F / 32});
  return std::max(1, std::min({8, 160 / rb, F / 32}));
}

// What the self-attention of a step reads besides the step's rows: the beam's cache slot ancestry, or, for
// greedy rows (one row per chunk, no ancestry), the tokens picked so far, c->gtok with leading dimension
// gtok_ld = the call's max_len (0: the cache), by which layer 0 reads its history from the table; and the
// previous step's greedy head, fused into layer 0
struct StepHist {
  const int* anc = nullptr;
  int anc_ld = 0;
  int gtok_ld = 0;
  const nd::GreedyHead* head = nullptr;
};

// rows: C chunks of rpc rows; rows.done (--fast beam; null otherwise): the finished chunks' tiles and
// attention workgroups exit without work
static hipError_t enqueue_dec_step(nd_ctx* c, const nd::RowSet& rows, int T, int step, const StepHist& h,
                                   hipStream_t s) {
  const int C = rows.C, rpc = rows.rpc, R = C * rpc, D = c->D, F = c->F, S = c->cfg.max_steps;
  const int* const done = rows.done;
  const int Ld = (int)c->m.dec.size();
  const bool mb = use_memory_bank(c, rpc);
  int pnx = 1, pnq = 0, pnm = 0;
  // a decoder-step GEMM over the R rows: P16 operands, split-fp16 weights, dead chunks skipped
  auto dg = [&](const float* A, int lda, const float* W, int N, int K, const float* bias, float* out, int ldc) {
    return G(A, lda, W, N, K, bias, out, ldc, R).p16().h3(c).skip(done, rpc).small_m(c->beam_tail).splitk(c);
  };
  const nd::SrcMask mask{.signal = c->sig, .span = c->span, .pad_val = (float)c->cfg.pad_idx};
  for (int i = 0; i < Ld; ++i) {
    DecLayer& L = c->m.dec[i];
    // the self-attention history: beam rows keep 24-bit rows (1600 B per key, attention.hip
    // SELF_Q24_ROW) outside exact fp32; greedy rows, exact fp32 and the average-attention layers keep
    // fp32 k | v (2 KB).  Same box, two reps (profiles/r05_self_q24_ab.txt): configs[3] pooled
    // 67.71 / 67.78 -> 67.28 / 67.17 ms; greedy configs[1] pooled 15.55 / 15.53 -> 15.70 / 15.74 (the
    // row's own history is 100 keys at most: the dequantise costs more than the bytes it saves)
    const bool sq24 = h.anc && !c->exact && c->cfg.self_attn_type != ND_SELF_AVERAGE;
    float* cache = sq24 ? reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(c->cache) + (size_t)i * R * S * CTXQ_ROW)
                        : c->cache + (size_t)i * R * S * 2 * D;
    // kernel stamps; -attn_debug (greedy): the last layer's head-0 context scores, [B][S][T]
    const nd::AttnTap tap{.stamp = c->kstamp_on ? c->kstamp + 2 * ((size_t)step * Ld + i) : nullptr,
                          .dbg = (c->attn_on && i == Ld - 1) ? c->attn_raw + (size_t)step * T : nullptr,
                          .dbg_stride = (size_t)S * T};
    // decoder/transformer.py:53-95
    // all step activations are P16-packed (kernels.hpp)
    if (c->cfg.self_attn_type == ND_SELF_AVERAGE) {
      // average_attn.py:55-106 + the layer residual (decoder/transformer.py:82-86)
      LCHK(nd::launch_aan_prep({.x = c->dx, .ln_g = L.ln1_g, .ln_b = L.ln1_b, .hist = cache, .anc = h.anc,
                                .anc_ld = h.anc_ld, .step = step, .max_steps = S, .xn = c->axn, .avg = c->aavg,
                                .avg_part = c->aavg_part, .R = R}, s));
      LCHK(dg(c->aavg, D, L.paw1, D, D, L.nab1, c->ah, D).ln(c->aavg_part, 1).relu().run(s));
      LCHK(dg(c->ah, D, L.paw2, D, D, L.ab2, c->aa, D).res(c->aavg, D).run(s));
      LCHK(dg(c->axn, D, L.pgwx, 2 * D, D, L.gb, c->ag, 2 * D).run(s));
      LCHK(dg(c->aa, D, L.pgwa, 2 * D, D, nullptr, c->ag, 2 * D).res(c->ag, 2 * D).run(s));
      LCHK(nd::launch_aan_gate(c->ag, c->axn, c->aa, c->dx, c->dq1, c->dq1_part, R, s));
      pnq = 1;
    } else {
      nd::SelfAttnArgs sa{.qkv = c->dqkv, .cache = cache, .anc = h.anc, .anc_ld = h.anc_ld, .step = step,
                          .max_steps = S, .out = c->datt, .R = R, .rows = rows, .q24 = sq24};
      if (i == 0 && qkv_table(c)) {  // the row's q | k | v from the model's table
        sa.qkv = qkv_table(c);
        sa.qr.tok = c->rtok;
        sa.qr.V = c->V;
        sa.qr.tok0 = c->cfg.bos_idx;
        sa.qr.rm = 1;  // the table is row-major (model.hip build_qkv_tables)
        if (h.gtok_ld > 0 && rpc == 1 && !h.anc && !done && !rows.clist) {  // greedy rows: the history too
          sa.qr.hist = c->gtok;
          sa.qr.hist_ld = h.gtok_ld;
        }
        sa.head = h.head;
      } else {
        // greedy rows (one workgroup each): q | k | v row-major; beam keeps P16 (its M = 5120 GEMMs
        // take the LDS-tiled route, which writes P16)
        sa.qr.rm = (rpc == 1 && !h.anc && !done) ? 1 : 0;
        LCHK(dg(c->dx, D, L.pwqkv, 3 * D, D, L.nbqkv, c->dqkv, 3 * D).ln(c->dx_part, pnx).c_rowmajor(sa.qr.rm).run(s));
      }
      LCHK(nd::launch_dec_self_attention(sa, s));
      LCHK(dg(c->datt, D, L.pwo, D, D, L.bo, c->dq1, D).res(c->dx, D).stats(c->dq1_part).run(s, &pnq));
    }
    if (mb) {  // memory-bank form (attention.hip)
      const int HD = ND_H * D;
      // q' row-major for the digit-bank kernel (one row per chunk), P16 for the fp32 one
      LCHK(dg(c->dq1, D, L.pwqk, HD, D, L.bqk, c->dqk, HD).ln(c->dq1_part, pnq).c_rowmajor(c->bank_d8).run(s));
      if (c->bank_d8)
        LCHK(nd::launch_dec_bank_d8({.qp = c->dqk, .bank = c->mem_p, .kscale = c->bank_ks, .kemax = c->bank_em,
                                     .mask = mask, .out = c->dU, .C = C, .T = T, .tap = tap, .ovf = c->ovf,
                                     .nt = c->bank_nt, .grid = c->bank_grid}, s));
      else
        LCHK(nd::launch_dec_mem_attention({.qp = c->dqk, .mem = c->mem, .mask = mask, .out = c->dU, .C = C, .rpc = rpc,
                                           .T = T, .ldT = T, .tap = tap, .grid = c->bank_grid}, s));
      LCHK(dg(c->dU, HD, L.pwvo, D, HD, L.bvo, c->dmid, D).res(c->dq1, D).stats(c->dmid_part).run(s, &pnm));
    } else {
      LCHK(dg(c->dq1, D, L.pcwq, D, D, L.ncbq, c->dcq, D).ln(c->dq1_part, pnq).run(s));
      // beam rows read layer i's plane of the 24-bit image (ld, koff in bytes), or its columns of the fp32 K/V
      nd::CtxAttnArgs ca{.q = c->dcq, .kv = c->ctxkv, .ld = Ld * 2 * D, .koff = i * 2 * D, .q24 = c->ctx_q24, .T = T,
                         .out = c->datt, .mask = mask, .rows = rows, .tap = tap, .nsplit = ctx_split(),
                         .part = c->ctx_part};
      if (c->ctx_q24) {
        ca.kv = c->ctxq + (size_t)i * C * T * CTXQ_ROW;
        ca.ld = CTXQ_ROW;
        ca.koff = 0;
      }
      LCHK(nd::launch_dec_ctx_attention(ca, s));
      LCHK(dg(c->datt, D, L.pcwo, D, D, L.cbo, c->dmid, D).res(c->dq1, D).stats(c->dmid_part).run(s, &pnm));
    }
    if (const int ns = dec_ffn_splits(c, R)) {  // beam rows: the fused block, hidden on chip (ffn.hip)
      const auto& i1 = c->m.split.at(L.pw1);
      const auto& i2 = c->m.split.at(L.pw2);
      LCHK(nd::launch_dec_ffn({.y = c->dmid, .w1h = i1.first, .w1s = i1.second, .b1 = L.nb1, .w2h = i2.first,
                               .w2s = i2.second, .b2 = L.b2, .x = c->dx, .xpart = c->dx_part, .M = R, .F = F,
                               .ovf = c->ovf},
                              {.nsplit = ns, .slab = c->dffn_slab, .tickets = c->dffn_cnt, .skip = done,
                               .skip_rpc = rpc}, s));
      pnx = 1;  // each row's exact statistics in one partial
    } else {
      LCHK(dg(c->dmid, D, L.pw1, F, D, L.nb1, c->dhid, F).ln(c->dmid_part, pnm).relu().run(s));
      LCHK(dg(c->dhid, F, L.pw2, D, F, L.b2, c->dx, D).res(c->dmid, D).stats(c->dx_part).run(s, &pnx));
    }
  }
  return hipSuccess;
}

// The decoder's view of the encoder output: the memory bank (greedy) or the
// per-layer context K/V (beam).
static hipError_t enqueue_memory(nd_ctx* c, int B, int T, int rpc, hipStream_t s) {
  set_memory_view(c, T, rpc);
  if (!use_memory_bank(c, rpc)) {
    if (!c->ctxkv) return hipErrorInvalidValue;  // a beam call on a context created with max_beam 1
    // the 24-bit image comes straight from the K/V GEMM's epilogue; it needs the split-fp16 weights (h3), and
    // exact fp32 never takes the image
    return enqueue_ctxkv(c, B, T, s, c->ctx_q24);
  }
  const bool tf = c->cfg.encoder_type == ND_ENC_TRANSFORMER;
  if (c->bank_d8)
    return nd::launch_bank_pack_d8({.x = c->x, .ln_g = tf ? c->m.bank_ln_g : nullptr,
                                    .ln_b = tf ? c->m.bank_ln_b : nullptr, .bank = c->mem_p, .kscale = c->bank_ks,
                                    .kemax = c->bank_em, .span = c->span, .B = B, .T = T, .ovf = c->ovf}, s);
  if (!tf) return hipSuccess;  // the NanoEncoder's output is the bank as it stands
  return nd::launch_memory_pack(c->x, c->m.bank_ln_g, c->m.bank_ln_b, c->mem_p, B, T, T, s);
}

static hipError_t enqueue_greedy(nd_ctx* c, int B, int T, int S, int min_len, bool logp, const nd::Sampling& smp,
                                 hipStream_t s) {
  if (c->kstamp_on) LCHK(nd::launch_stamp_reset(c->kstamp, (int)c->m.dec.size() * c->cfg.max_steps, s));
  LCHK(enqueue_encode(c, B, T, s));
  LCHK(enqueue_memory(c, B, T, 1, s));
  LCHK(nd::launch_fill_i32(c->tok, c->cfg.bos_idx, B, s));
  LCHK(enqueue_first_embed(c, B, s));
  // step k's head runs inside step k + 1's layer-0 self-attention (table
  // mode); only the last step's head is a launch of its own
  const bool fuse = head_fused(c);
  const nd::GreedyHead hd{.x = c->dx, .ln_g = c->m.dec_ln_g, .ln_b = c->m.dec_ln_b, .gw = c->m.gen_w, .gb = c->m.gen_b,
                          .V = c->V, .S = S, .min_len = min_len, .eos = c->cfg.eos_idx, .tok = c->tok,
                          .out_tokens = c->gtok, .score = c->gscore, .logp_dump = logp ? c->glogp : nullptr,
                          .ne = next_embed(c), .smp = smp};
  const nd::RowSet rows{.C = B, .rpc = 1};
  for (int step = 0; step < S; ++step) {
    LCHK(enqueue_dec_step(c, rows, T, step, {.gtok_ld = S, .head = fuse && step > 0 ? &hd : nullptr}, s));
    if (!fuse || step == S - 1) LCHK(nd::launch_dec_greedy_head(hd, step, B, s));
  }
  if (c->attn_on) LCHK(nd::launch_attn_rows_softmax(c->attn_raw, c->span, B, c->cfg.max_steps, T, s));
  return hipSuccess;
}

// the beam paths' view of the search state: the attention rows are visible
// to the search kernels only while a capturing call is enqueued
static nd::BeamState beam_state(nd_ctx* c) {
  nd::BeamState st = c->bs;
  st.attn = c->attn_on ? c->attn_raw : nullptr;
  st.cut = c->cut_in;
  return st;
}

// -attn_debug / coverage: this step's captured scores -> probabilities
static hipError_t enqueue_attn_step(nd_ctx* c, int C, int rpc, int T, int step, hipStream_t s) {
  if (!c->attn_on) return hipSuccess;
  const size_t S = c->cfg.max_steps;
  return nd::launch_attn_step_softmax(c->attn_raw + (size_t)step * T, S * T, c->span, C * rpc, rpc, T, s);
}

// the output head over the decoder rows x
static nd::Generator generator(const nd_ctx* c, const float* x) {
  return {.x = x, .ln_g = c->m.dec_ln_g, .ln_b = c->m.dec_ln_b, .gw = c->m.gen_w, .gb = c->m.gen_b, .V = c->V};
}

static hipError_t enqueue_beam_steps(nd_ctx* c, int B, int T, int beam, int n_best, float alpha, int S, int min_len,
                                     int s0, int s1, hipStream_t s) {
  const nd::BeamState st = beam_state(c);
  nd::BeamCall bc{.rows = {.C = B, .rpc = beam, .done = c->bs.done}, .n_best = n_best, .S = S, .min_len = min_len,
                  .eos = c->cfg.eos_idx};
  // the tail (at most a sixteenth of the chunks alive, translate_beam): the attention and beam-step launches
  // run over the segment's alive chunks only (a list built at its start), not B chunks that exit at once
  if (c->beam_tail) {
    bc.rows.clist = c->clist;
    bc.rows.ccap = (B + 15) / 16;
    LCHK(nd::launch_alive_list(c->bs.done, B, c->clist, bc.rows.ccap, c->ovf, s));
  }
  for (int step = s0; step < s1; ++step) {
    LCHK(enqueue_dec_step(c, bc.rows, T, step, {.anc = c->bs.anc[step & 1], .anc_ld = S}, s));
    LCHK(enqueue_attn_step(c, B, beam, T, step, s));
    LCHK(nd::launch_beam_step(next_embed(c), generator(c, c->dx), st, bc, step, nd::fast_beam_lenpen(step, alpha), s));
  }
  return hipSuccess;
}

static hipError_t enqueue_classic_steps(nd_ctx* c, int B, int T, int beam, int n_best, const nd::ClassicOpts& o, int S,
                                        int min_len, int s0, int s1, hipStream_t s) {
  const nd::BeamState st = beam_state(c);
  const nd::BeamCall bc{.rows = {.C = B, .rpc = beam}, .n_best = n_best, .S = S, .min_len = min_len,
                        .eos = c->cfg.eos_idx};
  for (int step = s0; step < s1; ++step) {
    LCHK(enqueue_dec_step(c, bc.rows, T, step, {.anc = c->bs.anc[step & 1], .anc_ld = S}, s));
    LCHK(enqueue_attn_step(c, B, beam, T, step, s));
    LCHK(nd::launch_beam_classic_step(next_embed(c), generator(c, c->dx), st, bc, step, o, s));
  }
  return hipSuccess;
}

// --------------------------------------------------------------- graphs
void drop_graphs(nd_ctx* c) {
  for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second);
  c->graphs.clear();
}

template <typename F>
static int run_graph(nd_ctx* c, const GraphKey& key, F&& enqueue) {
  if (!c->use_graphs) {
    hipError_t e = enqueue(c->es);
    if (e != hipSuccess) return fail(ND_ERR_HIP, g_err.empty() ? hipGetErrorString(e) : g_err);
    return ND_OK;
  }
  GraphKey k = key;
  k.stamp = c->kstamp_on ? 1 : 0;
  k.exact = c->exact ? 1 : 0;  // both product forms keep their graphs (the overflow rerun switches)
  k.tail = c->beam_tail ? 1 : 0;
  k.bank_nt = c->bank_nt ? 1 : 0;
  k.bank_grid = c->bank_grid;
  k.splitk = c->splitk ? 1 : 0;
  auto it = c->graphs.find(k);
  if (it == c->graphs.end()) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(c->es, hipStreamCaptureModeRelaxed));
    hipError_t e = enqueue(c->es);
    hipError_t e2 = hipStreamEndCapture(c->es, &g);
    if (e != hipSuccess) {
      if (g) (void)hipGraphDestroy(g);
      return fail(ND_ERR_HIP, "capture: " + g_err);
    }
    if (e2 != hipSuccess) return fail(ND_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e2));
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail(ND_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    it = c->graphs.emplace(k, ex).first;
  }
  HIPCHK(hipGraphLaunch(it->second, c->es));
  return ND_OK;
}

// --------------------------------------------------------------- C-ABI
// (the nd_* functions take their C linkage from their declarations in nanodec.h)
const char* nd_last_error(void) { return g_err.c_str(); }
const char* nd_version(void) { return "nanodec_hip 0.1.0 gfx950 fp32-mfma"; }

// Engine streams are recycled, never destroyed: a caller may still hold HIP
// events recorded on a context's stream (EnginePool results carry one) after
// the context is gone, and destroying the stream under them leaves the
// events pointing at a freed queue.  nd_destroy parks its (synchronised)
// stream here; nd_create takes a parked one first.
static std::mutex g_streams_mu;
static std::vector<std::pair<int, hipStream_t>> g_spare_streams;  // (device, stream)

static hipError_t acquire_stream(int dev, hipStream_t* s) {
  {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    for (size_t i = 0; i < g_spare_streams.size(); ++i)
      if (g_spare_streams[i].first == dev) {
        *s = g_spare_streams[i].second;
        g_spare_streams.erase(g_spare_streams.begin() + i);
        return hipSuccess;
      }
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

static void release_stream(int dev, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  g_spare_streams.emplace_back(dev, s);
}

int nd_create(const nd_config* cfg, nd_ctx** out) {
  if (!cfg || !out) return fail(ND_ERR_ARG, "null argument");
  *out = nullptr;
  if (cfg->d_model != ND_D || cfg->heads != ND_H) return fail(ND_ERR_ARG, "only d_model=256, heads=8 are compiled");
  if (cfg->d_ff <= 0 || cfg->d_ff % 128) return fail(ND_ERR_ARG, "d_ff must be a positive multiple of 128");
  if (cfg->vocab < 4 || cfg->vocab > ND_MAXV) return fail(ND_ERR_ARG, "vocab must be in [4, 32]");
  if (cfg->max_src_len < 1 || cfg->max_src_len > 512) return fail(ND_ERR_ARG, "max_src_len must be in [1, 512]");
  if (cfg->max_steps < 1 || cfg->max_steps > 512) return fail(ND_ERR_ARG, "max_steps must be in [1, 512]");
  if (cfg->max_beam < 1 || cfg->max_beam > 8) return fail(ND_ERR_ARG, "max_beam must be in [1, 8]");
  if (cfg->max_batch < 1) return fail(ND_ERR_ARG, "max_batch must be >= 1");
  if (cfg->enc_layers < 1 || cfg->dec_layers < 1) return fail(ND_ERR_ARG, "layers must be >= 1");
  if (cfg->encoder_type != ND_ENC_TRANSFORMER && cfg->encoder_type != ND_ENC_NANO)
    return fail(ND_ERR_ARG, "unknown encoder_type");
  if (cfg->encoder_type == ND_ENC_NANO && cfg->rnn_hidden != 128) return fail(ND_ERR_ARG, "rnn_hidden must be 128");
  if (cfg->self_attn_type != ND_SELF_SCALED_DOT && cfg->self_attn_type != ND_SELF_AVERAGE)
    return fail(ND_ERR_ARG, "unknown self_attn_type");
  HIPCHK(hipSetDevice(cfg->device));
  nd_ctx* c = new nd_ctx();
  c->cfg = *cfg;
  c->F = cfg->d_ff;
  c->V = cfg->vocab;
  c->H = cfg->rnn_hidden;
  int rc = build_registry(c);
  if (rc == ND_OK) rc = alloc_workspaces(c);
  if (rc != ND_OK) {
    nd_destroy(c);
    return rc;
  }
  hipError_t e = nd::init_kernel_attributes();
  if (e == hipSuccess) e = acquire_stream(cfg->device, &c->es);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreate(&c->ev_a);
  if (e == hipSuccess) e = hipEventCreate(&c->ev_b);
  if (e == hipSuccess) e = hipEventCreate(&c->ev_c);
  if (e != hipSuccess) {
    nd_destroy(c);
    return fail(ND_ERR_HIP, std::string("stream/event setup: ") + hipGetErrorString(e));
  }
  *out = c;
  return ND_OK;
}

static int check_call(nd_ctx* c, int B, int T, int S) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  if (!c->finalized) return fail(ND_ERR_STATE, "nd_finalize has not been called");
  if (B < 1 || B > c->cfg.max_batch) return fail(ND_ERR_ARG, "B out of range [1, max_batch]");
  if (T < 1 || T > c->cfg.max_src_len) return fail(ND_ERR_ARG, "T out of range [1, max_src_len]");
  if (S < 1 || S > c->cfg.max_steps) return fail(ND_ERR_ARG, "max_len out of range [1, max_steps]");
  return ND_OK;
}

static int stage_inputs(nd_ctx* c, const float* sig, const int32_t* len, const int32_t* span, int B, int T,
                        hipStream_t cs) {
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipEventRecord(c->ev_in, cs));
  HIPCHK(hipStreamWaitEvent(c->es, c->ev_in, 0));
  HIPCHK(hipMemcpyAsync(c->sig, sig, (size_t)B * T * 4, hipMemcpyDeviceToDevice, c->es));
  HIPCHK(hipMemcpyAsync(c->len, len, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  HIPCHK(hipMemcpyAsync(c->span, span, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  return ND_OK;
}

static int release_to(nd_ctx* c, hipStream_t cs) {
  HIPCHK(hipEventRecord(c->ev_out, c->es));
  HIPCHK(hipStreamWaitEvent(cs, c->ev_out, 0));
  return ND_OK;
}

// the attention capture buffer, [decoder rows][max_steps][max_src_len], made on first use
static int ensure_attn(nd_ctx* c) {
  if (c->attn_raw) return ND_OK;
  const size_t R = ((size_t)c->cfg.max_batch * std::max(1, c->cfg.max_beam) + 15) / 16 * 16;
  hipError_t e = dalloc(c, &c->attn_raw, R * c->cfg.max_steps * c->cfg.max_src_len);
  if (e != hipSuccess) return fail(ND_ERR_HIP, std::string("hipMalloc attention capture: ") + hipGetErrorString(e));
  return ND_OK;
}

// The per-call flags live on the context while a call's graphs are enqueued or captured (the enqueue
// functions and run_graph's key read them) and are cleared on every way out of the driver.
struct CallFlags {
  nd_ctx* c;
  CallFlags(nd_ctx* ctx, bool attn) : c(ctx) {
    c->attn_on = attn;
    c->beam_tail = false;
  }
  ~CallFlags() { c->attn_on = c->beam_tail = false; }
  CallFlags(const CallFlags&) = delete;
  CallFlags& operator=(const CallFlags&) = delete;
};

static int translate_greedy(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                            int32_t T, int32_t max_len, int32_t min_len, int32_t* d_tokens, float* d_score,
                            float* d_logp, float* d_attn, void* stream, float temp = 0.f, int topk = 1,
                            unsigned long long seed = 0) {
  int rc = check_call(c, B, T, max_len);
  if (rc) return rc;
  if (!d_signal || !d_len || !d_span || !d_tokens || !d_score) return fail(ND_ERR_ARG, "null buffer");
  if (d_attn && (rc = ensure_attn(c))) return rc;
  hipStream_t cs = (hipStream_t)stream;
  if ((rc = stage_inputs(c, d_signal, d_len, d_span, B, T, cs))) return rc;
  const bool lp = d_logp != nullptr;
  GraphKey key;
  key.mode = 0;
  key.B = B;
  key.T = T;
  key.S = max_len;
  key.min_len = min_len;
  key.attn = d_attn ? 1 : 0;
  key.logp = lp ? 1 : 0;
  nd::Sampling smp;
  if (temp != 0.f && topk != 1) {  // sample_with_temperature's random branch (translator.py:376-393)
    smp.temp = temp;
    smp.topk = topk;
    smp.seed = c->seed_dev;
    key.topk = topk;
    key.temp = temp;
    // the seed travels as kernel arguments (captured at launch), not through host memory
    int* sw = reinterpret_cast<int*>(c->seed_dev);
    HIPCHK(nd::launch_fill_i32(sw, (int)(unsigned)(seed & 0xffffffffull), 1, c->es));
    HIPCHK(nd::launch_fill_i32(sw + 1, (int)(unsigned)(seed >> 32), 1, c->es));
  }
  if (c->timing) HIPCHK(hipEventRecord(c->ev_a, c->es));
  {
    const CallFlags flags(c, d_attn != nullptr);
    set_memory_view(c, T, 1);
    rc = run_graph(c, key, [&](hipStream_t s) { return enqueue_greedy(c, B, T, max_len, min_len, lp, smp, s); });
  }
  if (rc) return rc;
  if (c->timing) HIPCHK(hipEventRecord(c->ev_b, c->es));
  HIPCHK(hipMemcpyAsync(d_tokens, c->gtok, (size_t)B * max_len * 4, hipMemcpyDeviceToDevice, c->es));
  HIPCHK(hipMemcpyAsync(d_score, c->gscore, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  if (lp) HIPCHK(hipMemcpyAsync(d_logp, c->glogp, (size_t)B * max_len * c->V * 4, hipMemcpyDeviceToDevice, c->es));
  if (d_attn)  // [B][max_steps][T] -> [B][max_len][T]
    HIPCHK(hipMemcpy2DAsync(d_attn, (size_t)max_len * T * 4, c->attn_raw, (size_t)c->cfg.max_steps * T * 4,
                            (size_t)max_len * T * 4, B, hipMemcpyDeviceToDevice, c->es));
  if (c->timing) {
    HIPCHK(hipEventSynchronize(c->ev_b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
    c->t_enc = 0.f;
    c->t_dec = ms;
  }
  return release_to(c, cs);
}

int nd_translate_greedy(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                        int32_t T, int32_t max_len, int32_t min_len, int32_t* d_tokens, float* d_score, float* d_logp,
                        void* stream) {
  return translate_greedy(c, d_signal, d_len, d_span, B, T, max_len, min_len, d_tokens, d_score, d_logp, nullptr,
                          stream);
}

int nd_translate_greedy_attn(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                             int32_t B, int32_t T, int32_t max_len, int32_t min_len, int32_t* d_tokens, float* d_score,
                             float* d_logp, float* d_attn, void* stream) {
  if (!d_attn) return fail(ND_ERR_ARG, "null attention buffer");
  return translate_greedy(c, d_signal, d_len, d_span, B, T, max_len, min_len, d_tokens, d_score, d_logp, d_attn,
                          stream);
}

// The segmented beam driver shared by the --fast beam and the classic Beam: the checks, input staging, the
// prologue graph (encoder, memory, search init), the decoder steps in graphs of SEG steps with a poll of the
// alive count between them, then finish and the attention gather.  key carries the call's shape and options
// (seg is filled here; key.attn: the call captures the attention).  init / steps / finish are the search's own
// launches.  tail: once a sixteenth of the chunks or fewer are alive, the remaining segments run on the tail
// kernels (--fast; the classic Beam never does).
struct BeamIo {
  const float* d_signal;
  const int32_t *d_len, *d_span;
  const int32_t *d_group, *d_cut;  // the classic Beam's reference-batch ids and attention lengths (nullable)
  int32_t* d_tokens;
  float* d_scores;
  int32_t *d_lens, *d_steps;
  float* d_attn;
  int32_t* d_done_step;
  void* stream;
};

template <typename Init, typename Steps, typename Finish>
static int translate_segmented(nd_ctx* c, const BeamIo& io, GraphKey key, bool tail, Init&& init, Steps&& steps,
                               Finish&& finish) {
  const int B = key.B, T = key.T, beam = key.beam, n_best = key.n_best, max_len = key.S;
  int rc = check_call(c, B, T, max_len);
  if (rc) return rc;
  if (beam < 1 || beam > c->cfg.max_beam) return fail(ND_ERR_ARG, "beam out of range [1, max_beam]");
  if (n_best < 1 || n_best > beam) return fail(ND_ERR_ARG, "n_best out of range [1, beam]");
  if (c->V < beam) return fail(ND_ERR_ARG, "vocab smaller than beam");
  if (!io.d_signal || !io.d_len || !io.d_span || !io.d_tokens || !io.d_scores || !io.d_lens)
    return fail(ND_ERR_ARG, "null buffer");
  if (key.attn && (rc = ensure_attn(c))) return rc;
  hipStream_t cs = (hipStream_t)io.stream;
  if ((rc = stage_inputs(c, io.d_signal, io.d_len, io.d_span, B, T, cs))) return rc;
  if (io.d_group) HIPCHK(hipMemcpyAsync(c->group_in, io.d_group, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  if (io.d_cut) HIPCHK(hipMemcpyAsync(c->cut_in, io.d_cut, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  // n_best hypothesis storage is sized by max_beam
  const int SEG = 10;
  if (c->timing) HIPCHK(hipEventRecord(c->ev_a, c->es));
  {
    const CallFlags flags(c, key.attn != 0);
    set_memory_view(c, T, beam);
    key.seg = -1;
    rc = run_graph(c, key, [&](hipStream_t s) -> hipError_t {
      if (c->kstamp_on) LCHK(nd::launch_stamp_reset(c->kstamp, (int)c->m.dec.size() * c->cfg.max_steps, s));
      LCHK(enqueue_encode(c, B, T, s));
      LCHK(enqueue_memory(c, B, T, beam, s));  // K/V per layer (memory bank at beam 1)
      LCHK(init(s));
      LCHK(enqueue_first_embed(c, B * beam, s));
      LCHK(nd::launch_fill_i32(c->steps_done, max_len, 1, s));
      return hipSuccess;
    });
    if (rc) return rc;
    if (c->timing) HIPCHK(hipEventRecord(c->ev_b, c->es));
    for (int s0 = 0; s0 < max_len; s0 += SEG) {
      const int s1 = std::min(max_len, s0 + SEG);
      key.seg = s0;
      rc = run_graph(c, key, [&](hipStream_t s) { return steps(s0, s1, s); });
      if (rc) return rc;
      if (s1 < max_len) {
        HIPCHK(hipMemcpyAsync(c->h_alive, c->bs.n_alive, 4, hipMemcpyDeviceToHost, c->es));
        HIPCHK(hipStreamSynchronize(c->es));
        if (*c->h_alive == 0) break;
        // a sixteenth of the chunks or fewer left (a trained model's stragglers):
        // the remaining segments' GEMMs run on the latency-bound small-M kernels
        c->beam_tail = tail && (long)*c->h_alive * 16 <= (long)B;
      }
    }
  }
  if (c->timing) HIPCHK(hipEventRecord(c->ev_c, c->es));
  HIPCHK(finish(c->es));
  if (io.d_steps) HIPCHK(hipMemcpyAsync(io.d_steps, c->steps_done, 4, hipMemcpyDeviceToDevice, c->es));
  if (io.d_attn) {
    nd::BeamState bst = c->bs;
    bst.attn = c->attn_raw;
    HIPCHK(nd::launch_beam_attn_gather(bst, B, n_best, c->cfg.max_steps, max_len, T, io.d_attn, c->es));
  }
  if (io.d_done_step)
    HIPCHK(hipMemcpyAsync(io.d_done_step, c->bs.steps_run, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  if (c->timing) {
    HIPCHK(hipEventSynchronize(c->ev_c));
    HIPCHK(hipEventElapsedTime(&c->t_enc, c->ev_a, c->ev_b));
    HIPCHK(hipEventElapsedTime(&c->t_dec, c->ev_b, c->ev_c));
  }
  return release_to(c, cs);
}

static int translate_beam(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                          int32_t T, int32_t beam, int32_t n_best, float alpha, int32_t max_len, int32_t min_len,
                          int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, float* d_attn,
                          int32_t* d_done_step, void* stream) {
  const BeamIo io{d_signal, d_len, d_span, nullptr, nullptr, d_tokens, d_scores,
                  d_lens,   d_steps, d_attn, d_done_step, stream};
  GraphKey key;
  key.mode = 1;
  key.B = B;
  key.T = T;
  key.S = max_len;
  key.min_len = min_len;
  key.beam = beam;
  key.n_best = n_best;
  key.alpha = alpha;
  key.attn = d_attn ? 1 : 0;
  return translate_segmented(
      c, io, key, true,
      [&](hipStream_t s) { return nd::launch_beam_init(c->bs, B, beam, c->cfg.bos_idx, s); },
      [&](int s0, int s1, hipStream_t s) {
        return enqueue_beam_steps(c, B, T, beam, n_best, alpha, max_len, min_len, s0, s1, s);
      },
      [&](hipStream_t s) { return nd::launch_beam_finish(c->bs, B, n_best, max_len, d_tokens, d_scores, d_lens, s); });
}

int nd_translate_sample(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                        int32_t T, int32_t max_len, int32_t min_len, float temp, int32_t keep_topk, uint64_t seed,
                        int32_t* d_tokens, float* d_score, float* d_logp, float* d_attn, void* stream) {
  if (keep_topk > c->V) return fail(ND_ERR_ARG, "random_sampling_topk larger than the vocabulary");
  return translate_greedy(c, d_signal, d_len, d_span, B, T, max_len, min_len, d_tokens, d_score, d_logp, d_attn,
                          stream, temp, keep_topk, (unsigned long long)seed);
}

int nd_translate_beam(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                      int32_t T, int32_t beam, int32_t n_best, float alpha, int32_t max_len, int32_t min_len,
                      int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, void* stream) {
  return translate_beam(c, d_signal, d_len, d_span, B, T, beam, n_best, alpha, max_len, min_len, d_tokens, d_scores,
                        d_lens, d_steps, nullptr, nullptr, stream);
}

int nd_translate_beam_attn(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                           int32_t T, int32_t beam, int32_t n_best, float alpha, int32_t max_len, int32_t min_len,
                           int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, float* d_attn,
                           int32_t* d_done_step, void* stream) {
  if (!d_attn || !d_done_step) return fail(ND_ERR_ARG, "null attention buffer");
  return translate_beam(c, d_signal, d_len, d_span, B, T, beam, n_best, alpha, max_len, min_len, d_tokens, d_scores,
                        d_lens, d_steps, d_attn, d_done_step, stream);
}

static int translate_classic(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                             const int32_t* d_group, const int32_t* d_cut, int32_t B, int32_t T, int32_t beam,
                             int32_t n_best, const nd_classic_opts& op, int32_t max_len, int32_t min_len,
                             int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, float* d_attn,
                             void* stream) {
  if (op.length_penalty < 0 || op.length_penalty > 2)
    return fail(ND_ERR_ARG, "length_penalty must be 0 (none), 1 (wu), 2 (avg)");
  if (op.coverage_penalty < 0 || op.coverage_penalty > 2)
    return fail(ND_ERR_ARG, "coverage_penalty must be 0 (none), 1 (wu), 2 (summary)");
  if (op.block_ngram_repeat < 0 || op.block_ngram_repeat > max_len)
    return fail(ND_ERR_ARG, "block_ngram_repeat out of range [0, max_len]");
  if (!d_group) return fail(ND_ERR_ARG, "null buffer");
  if (op.coverage_penalty != 0 && !d_cut) return fail(ND_ERR_ARG, "coverage penalty needs the attention lengths");
  const nd::ClassicOpts o{op.length_penalty, op.alpha, op.beta,          op.coverage_penalty,
                          op.stepwise_penalty, op.block_ngram_repeat, op.ignore_mask};
  const BeamIo io{d_signal, d_len, d_span, d_group, d_cut, d_tokens, d_scores, d_lens, d_steps, d_attn, nullptr, stream};
  GraphKey key;
  key.mode = 2;
  key.B = B;
  key.T = T;
  key.S = max_len;
  key.min_len = min_len;
  key.beam = beam;
  key.n_best = n_best;
  key.alpha = op.alpha;
  key.attn = (d_attn != nullptr || op.coverage_penalty != 0) ? 1 : 0;  // the coverage penalties read the attention
  key.lenpen = op.length_penalty;
  key.cov = op.coverage_penalty;
  key.stepwise = op.stepwise_penalty;
  key.ngram = op.block_ngram_repeat;
  key.excl = op.ignore_mask;
  key.beta = op.beta;
  return translate_segmented(
      c, io, key, false,
      [&](hipStream_t s) { return nd::launch_beam_classic_init(c->bs, c->group_in, B, beam, c->cfg.bos_idx, s); },
      [&](int s0, int s1, hipStream_t s) {
        return enqueue_classic_steps(c, B, T, beam, n_best, o, max_len, min_len, s0, s1, s);
      },
      [&](hipStream_t s) {
        return nd::launch_beam_classic_finish(c->bs, B, beam, n_best, max_len, o, d_tokens, d_scores, d_lens, s);
      });
}

int nd_translate_beam_classic(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                              const int32_t* d_group, int32_t B, int32_t T, int32_t beam, int32_t n_best,
                              int32_t length_penalty, float alpha, int32_t max_len, int32_t min_len,
                              int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, void* stream) {
  nd_classic_opts op{};
  op.length_penalty = length_penalty;
  op.alpha = alpha;
  return translate_classic(c, d_signal, d_len, d_span, d_group, nullptr, B, T, beam, n_best, op, max_len, min_len,
                           d_tokens, d_scores, d_lens, d_steps, nullptr, stream);
}

int nd_translate_beam_classic_ex(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                                 const int32_t* d_group, const int32_t* d_cut, int32_t B, int32_t T, int32_t beam,
                                 int32_t n_best, const nd_classic_opts* opts, int32_t max_len, int32_t min_len,
                                 int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, float* d_attn,
                                 void* stream) {
  if (!opts) return fail(ND_ERR_ARG, "null options");
  return translate_classic(c, d_signal, d_len, d_span, d_group, d_cut, B, T, beam, n_best, *opts, max_len, min_len,
                           d_tokens, d_scores, d_lens, d_steps, d_attn, stream);
}

// ------------------------------------------------------- teacher-forced scoring
// The scoring call's workspaces, made by the first call (a context that never scores pays nothing): the
// per-layer context K/V when the context has none (alloc_ctx_kv, as nd_set_ctx_path(1) does) and the
// [max_batch * max_steps, .] decoder rows.
static int alloc_score_ws(nd_ctx* c) {
  int rc = alloc_ctx_kv(c);
  if (rc != ND_OK) return rc;
  if (c->tf_score) return ND_OK;  // allocated last
  const auto& cfg = c->cfg;
  const size_t B = cfg.max_batch, S = cfg.max_steps, D = c->D, F = c->F;
  const size_t M = (B * S + 255) / 256 * 256;  // whole GEMM row tiles
  hipError_t e;
#define WST(ptr, n)                                       \
  if ((e = dalloc(c, &(ptr), (size_t)(n))) != hipSuccess) \
    return fail(ND_ERR_HIP, std::string("hipMalloc scoring workspace " #ptr ": ") + hipGetErrorString(e));
  WST(c->tf_x, M * D);
  WST(c->tf_q1, M * D);
  WST(c->tf_mid, M * D);
  WST(c->tf_cq, M * D);
  WST(c->tf_att, M * D);
  // q | k | v, then the FFN hidden: the encoder's `big` (free once the context K/V are projected) when it
  // holds max_batch * max_steps rows
  if (cfg.max_steps <= cfg.max_src_len) {
    c->tf_big = c->big;
  } else {
    WST(c->tf_big, M * std::max(F, 3 * D));
  }
  WST(c->tf_x_part, M * ND_PART_LD * 2);
  WST(c->tf_q1_part, M * ND_PART_LD * 2);
  WST(c->tf_mid_part, M * ND_PART_LD * 2);
  WST(c->tf_gold, B * S);
  WST(c->tf_gold_len, B);
  WST(c->tf_tok_logp, B * S);
  WST(c->tf_logp, B * S * (size_t)c->V);
  WST(c->tf_post, B);
  WST(c->tf_best, B);
  WST(c->tf_score, B);
#undef WST
  return ND_OK;
}

// Encoder, fp32 context K/V of every layer, then the decoder over the M = N * L target rows at once
// (decoder/transformer.py:53-95 with step = None): the row-major GEMMs of the encoder side (split-fp16
// images of the decoder's fp32 weights, or fp32 MFMA in exact mode: the same G calls) around the two
// attentions of score.hip; the FFN is the two GEMMs (its hidden in tf_big), in both product modes.
// K targets per chunk (nd_score_candidates; nd_score_targets is K = 1): the encoder
// and the context K/V run over the B chunks, everything that works on decoder rows over the N = B * K
// sequences of L rows, and the context attention, the one place a decoder row meets its chunk, takes the K
// candidates of chunk c as the K * L consecutive query rows they are.  post: the candidates' posterior
// and best behind the head (tf_gold_len holds the [B, K] candidate lengths).
// want_attn (nd_score_targets_attn, K = 1): the last layer's context attention is the tapped form, its head-0
// scores dense [B * L, T] in attn_raw (ensure_attn), turned into probabilities right behind it.
// part: 0 the whole call; a timed call (nd_set_timing) enqueues 1, the encoder side, and 2, the decoder
// side, with an event between them: the same launches in the same order.
static hipError_t enqueue_score(nd_ctx* c, int B, int T, int K, int L, bool want_tok, bool want_logp, bool want_attn,
                                bool post, int part, hipStream_t s) {
  const Model& m = c->m;
  const int N = B * K, M = N * L, D = c->D, F = c->F, Ld = (int)m.dec.size();
  const float pad = (float)c->cfg.pad_idx;
  if (part != 2) {
    LCHK(enqueue_encode(c, B, T, s));
    LCHK(enqueue_ctxkv(c, B, T, s, false));
  }
  if (part == 1) return hipSuccess;
  LCHK(nd::launch_tf_embed(c->tf_gold, c->cfg.bos_idx, c->V, m.emb, c->cfg.position_encoding ? m.pe : nullptr, c->tf_x,
                           c->tf_x_part, N, L, s));
  int pnx = 1, pnq = 0, pnm = 0;
  const auto tap_here = [&](int layer) { return want_attn && layer == Ld - 1; };
  for (int i = 0; i < Ld; ++i) {
    const DecLayer& Y = m.dec[i];
    LCHK(G(c->tf_x, D, Y.nwqkv, 3 * D, D, Y.nbqkv, c->tf_big, 3 * D, M).h3(c).ln(c->tf_x_part, pnx).run(s));
    LCHK(nd::launch_tf_attention({.q = c->tf_big, .ldq = 3 * D, .kv = c->tf_big, .ldkv = 3 * D, .koff = D, .voff = 2 * D,
                                  .out = c->tf_att, .B = N, .Lq = L, .Lk = L, .causal = true}, s));
    LCHK(G(c->tf_att, D, Y.wo, D, D, Y.bo, c->tf_q1, D, M).h3(c).res(c->tf_x, D).stats(c->tf_q1_part).run(s, &pnq));
    LCHK(G(c->tf_q1, D, Y.ncwq, D, D, Y.ncbq, c->tf_cq, D, M).h3(c).ln(c->tf_q1_part, pnq).run(s));
    LCHK(nd::launch_tf_attention({.q = c->tf_cq, .ldq = D, .kv = c->ctxkv, .ldkv = Ld * 2 * D, .koff = i * 2 * D,
                                  .voff = i * 2 * D + D, .mask = {.signal = c->sig, .span = c->span, .pad_val = pad},
                                  .out = c->tf_att, .B = B, .Lq = K * L, .Lk = T,
                                  .tap = tap_here(i) ? c->attn_raw : nullptr, .ld_tap = tap_here(i) ? T : 0}, s));
    if (tap_here(i)) LCHK(nd::launch_attn_rows_softmax(c->attn_raw, c->span, B, K * L, T, s));
    LCHK(G(c->tf_att, D, Y.cwo, D, D, Y.cbo, c->tf_mid, D, M).h3(c).res(c->tf_q1, D).stats(c->tf_mid_part).run(s, &pnm));
    LCHK(G(c->tf_mid, D, Y.nw1, F, D, Y.nb1, c->tf_big, F, M).h3(c).ln(c->tf_mid_part, pnm).relu().run(s));
    LCHK(G(c->tf_big, F, Y.w2, D, F, Y.b2, c->tf_x, D, M).h3(c).res(c->tf_mid, D).stats(c->tf_x_part).run(s, &pnx));
  }
  LCHK(nd::launch_score_head(generator(c, c->tf_x), c->tf_gold, c->tf_gold_len, N, L, c->tf_score,
                             want_tok ? c->tf_tok_logp : nullptr, want_logp ? c->tf_logp : nullptr, s));
  if (!post) return hipSuccess;
  return nd::launch_cand_posterior(c->tf_score, c->tf_gold_len, B, K, c->tf_score, c->tf_post, c->tf_best, s);
}

// What a scoring call writes: score is required; attn belongs to nd_score_targets_attn, post and best
// (both nullable) to nd_score_candidates.
struct ScoreOut {
  float *score = nullptr, *tok_logp = nullptr, *logp = nullptr, *attn = nullptr, *post = nullptr;
  int32_t* best = nullptr;
};

// nd_score_targets (cand and want_attn false, K = 1: o.attn unused, the call and its graph as they were before
// the tap and the candidates existed), nd_score_targets_attn (want_attn: o.attn required) and
// nd_score_candidates (cand: d_gold [B, K, L], d_gold_len [B, K] with 0 for an empty slot)
static int score_targets(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                         const int32_t* d_gold, const int32_t* d_gold_len, int32_t B, int32_t T, int32_t K, int32_t L,
                         const ScoreOut& o, bool want_attn, bool cand, void* stream) {
  // every argument check comes before the first HIP call
  const std::string who = cand ? "nd_score_candidates" : want_attn ? "nd_score_targets_attn" : "nd_score_targets";
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  if (c->cfg.self_attn_type == ND_SELF_AVERAGE)
    return fail(ND_ERR_ARG, who + ": average-attention decoders are not supported (teacher-forced average "
                                  "attention is a cumulative mean, a kernel this library does not have)");
  if (K < 1) return fail(ND_ERR_ARG, who + ": K out of range [1, max_batch / B]");
  if (L < 1 || L > c->cfg.max_steps) return fail(ND_ERR_ARG, who + ": L out of range [1, max_steps]");
  int rc = check_call(c, B, T, L);
  if (rc) return rc;
  if ((int64_t)B * K > c->cfg.max_batch) return fail(ND_ERR_ARG, who + ": B * K out of range [1, max_batch]");
  if (!d_signal || !d_len || !d_span || !d_gold || !d_gold_len || !o.score) return fail(ND_ERR_ARG, "null buffer");
  if (want_attn && !o.attn) return fail(ND_ERR_ARG, who + ": null d_attn");
  HIPCHK(hipSetDevice(c->cfg.device));
  if ((rc = alloc_score_ws(c))) return rc;
  // attn_raw holds at least max_batch * max_steps * max_src_len floats: the dense [B * L, T] tap fits
  if (want_attn && (rc = ensure_attn(c))) return rc;
  hipStream_t cs = (hipStream_t)stream;
  const int N = B * K;
  if ((rc = stage_inputs(c, d_signal, d_len, d_span, B, T, cs))) return rc;
  HIPCHK(hipMemcpyAsync(c->tf_gold, d_gold, (size_t)N * L * 4, hipMemcpyDeviceToDevice, c->es));
  HIPCHK(hipMemcpyAsync(c->tf_gold_len, d_gold_len, (size_t)N * 4, hipMemcpyDeviceToDevice, c->es));
  const bool tl = o.tok_logp != nullptr, lp = o.logp != nullptr;
  GraphKey key;
  key.mode = 3;
  key.B = B;
  key.T = T;
  key.S = L;
  key.K = cand ? K : 0;
  key.logp = (tl ? 1 : 0) | (lp ? 2 : 0);
  key.attn = want_attn ? 1 : 0;
  {
    const CallFlags flags(c, false);
    const auto run = [&](int part) {
      key.seg = part == 1 ? -1 : part;  // the whole call keeps the key it always had (seg 0)
      return run_graph(c, key,
                       [&](hipStream_t s) { return enqueue_score(c, B, T, K, L, tl, lp, want_attn, cand, part, s); });
    };
    if (!c->timing) {
      rc = run(0);
    } else {  // the same launches as two pieces, the encoder side and the decoder side, an event between
      HIPCHK(hipEventRecord(c->ev_a, c->es));
      if ((rc = run(1))) return rc;
      HIPCHK(hipEventRecord(c->ev_b, c->es));
      rc = run(2);
      if (!rc) HIPCHK(hipEventRecord(c->ev_c, c->es));
    }
  }
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(o.score, c->tf_score, (size_t)N * 4, hipMemcpyDeviceToDevice, c->es));
  if (tl) HIPCHK(hipMemcpyAsync(o.tok_logp, c->tf_tok_logp, (size_t)N * L * 4, hipMemcpyDeviceToDevice, c->es));
  if (lp) HIPCHK(hipMemcpyAsync(o.logp, c->tf_logp, (size_t)N * L * c->V * 4, hipMemcpyDeviceToDevice, c->es));
  if (want_attn)
    HIPCHK(hipMemcpyAsync(o.attn, c->attn_raw, (size_t)N * L * T * 4, hipMemcpyDeviceToDevice, c->es));
  if (cand && o.post) HIPCHK(hipMemcpyAsync(o.post, c->tf_post, (size_t)N * 4, hipMemcpyDeviceToDevice, c->es));
  if (cand && o.best) HIPCHK(hipMemcpyAsync(o.best, c->tf_best, (size_t)B * 4, hipMemcpyDeviceToDevice, c->es));
  if (c->timing) {
    HIPCHK(hipEventSynchronize(c->ev_c));
    HIPCHK(hipEventElapsedTime(&c->t_enc, c->ev_a, c->ev_b));
    HIPCHK(hipEventElapsedTime(&c->t_dec, c->ev_b, c->ev_c));
  }
  return release_to(c, cs);
}

int nd_score_targets(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                     const int32_t* d_gold, const int32_t* d_gold_len, int32_t B, int32_t T, int32_t L, float* d_score,
                     float* d_tok_logp, float* d_logp, void* stream) {
  return score_targets(c, d_signal, d_len, d_span, d_gold, d_gold_len, B, T, 1, L,
                       {.score = d_score, .tok_logp = d_tok_logp, .logp = d_logp}, false, false, stream);
}

int nd_score_targets_attn(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                          const int32_t* d_gold, const int32_t* d_gold_len, int32_t B, int32_t T, int32_t L,
                          float* d_score, float* d_tok_logp, float* d_logp, float* d_attn, void* stream) {
  return score_targets(c, d_signal, d_len, d_span, d_gold, d_gold_len, B, T, 1, L,
                       {.score = d_score, .tok_logp = d_tok_logp, .logp = d_logp, .attn = d_attn}, true, false, stream);
}

int nd_score_candidates(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                        const int32_t* d_cand, const int32_t* d_cand_len, int32_t B, int32_t T, int32_t K, int32_t L,
                        float* d_score, float* d_post, int32_t* d_best, float* d_tok_logp, float* d_logp,
                        void* stream) {
  return score_targets(c, d_signal, d_len, d_span, d_cand, d_cand_len, B, T, K, L,
                       {.score = d_score, .tok_logp = d_tok_logp, .logp = d_logp, .post = d_post, .best = d_best},
                       false, true, stream);
}

int nd_encode(nd_ctx* c, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B, int32_t T,
              float* d_memory, void* stream) {
  int rc = check_call(c, B, T, 1);
  if (rc) return rc;
  hipStream_t cs = (hipStream_t)stream;
  if ((rc = stage_inputs(c, d_signal, d_len, d_span, B, T, cs))) return rc;
  hipError_t e = enqueue_encode(c, B, T, c->es);
  if (e != hipSuccess) return fail(ND_ERR_HIP, g_err);
  if (c->cfg.encoder_type == ND_ENC_TRANSFORMER) {
    e = nd::launch_layernorm(c->x, c->m.enc_ln_g, c->m.enc_ln_b, d_memory, B * T, c->es);
    if (e != hipSuccess) return fail(ND_ERR_HIP, hipGetErrorString(e));
  } else {
    HIPCHK(hipMemcpyAsync(d_memory, c->x, (size_t)B * T * c->D * 4, hipMemcpyDeviceToDevice, c->es));
  }
  return release_to(c, cs);
}

void* nd_stream(nd_ctx* c) { return c ? (void*)c->es : nullptr; }

int nd_gemm_routes(int64_t* counts, int32_t n, int32_t reset) {
  if (!counts || n < 0) return fail(ND_ERR_ARG, "null argument");
  for (int r = 0; r < ND_ROUTE_N; ++r) {
    const long long v = nd::gemm_route_count(r, reset != 0);
    if (r < n) counts[r] = v;
  }
  return ND_OK;
}

int nd_switches(char* buf, int32_t len) {
  std::string out;
  int n = 0;
  for (const auto& sw : kSwitches) {
    const char* e = getenv(sw.name);
    if (!e || atoi(e) == sw.def) continue;
    out += (n ? ";" : "") + std::string(sw.name) + "=" + e;
    ++n;
  }
  if (buf && len > 0) {
    const size_t k = std::min(out.size(), (size_t)len - 1);
    memcpy(buf, out.data(), k);
    buf[k] = 0;
  }
  return n;
}

int nd_set_graphs(nd_ctx* c, int enable) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  c->use_graphs = enable != 0;
  return ND_OK;
}

int nd_set_ctx_path(nd_ctx* c, int path) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  if (path < 0 || path > 1) return fail(ND_ERR_ARG, "path must be 0 (auto) or 1 (K/V form)");
  if (path == 1) {  // a greedy-only context allocates the context K/V now (beam contexts have it)
    HIPCHK(hipSetDevice(c->cfg.device));
    const int rc = alloc_ctx_kv(c);
    if (rc != ND_OK) return rc;
  }
  if (c->ctx_path != path) {
    drop_graphs(c);
  }
  c->ctx_path = path;
  return ND_OK;
}

int nd_set_bank_policy(nd_ctx* c, int nontemporal) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  c->bank_nt = nontemporal != 0;  // graphs are keyed by it
  return ND_OK;
}

int nd_set_bank_grid(nd_ctx* c, int32_t workgroups) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  if (workgroups < 0) return fail(ND_ERR_ARG, "bank grid: workgroups must be >= 0");
  c->bank_grid = workgroups;  // graphs are keyed by it
  return ND_OK;
}

int nd_set_gemm_splitk(nd_ctx* c, int32_t on) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  c->splitk = on != 0;  // graphs are keyed by it
  return ND_OK;
}

int nd_set_exact_fp32(nd_ctx* c, int enable) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  c->exact = enable != 0;  // graphs are keyed by it
  return ND_OK;
}

int nd_take_overflow(nd_ctx* c, int32_t* d_out, void* stream) {
  if (!c || !d_out) return fail(ND_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  const hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(d_out, c->ovf, sizeof(int), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemsetAsync(c->ovf, 0, sizeof(int), s));
  return ND_OK;
}

int nd_set_timing(nd_ctx* c, int enable) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  c->timing = enable != 0;
  return ND_OK;
}

int nd_set_kernel_stamps(nd_ctx* c, int enable) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  c->kstamp_on = enable != 0;
  return ND_OK;
}

int nd_kernel_stamps(nd_ctx* c, float* avg_us, int32_t* launches) {
  if (!c || !avg_us || !launches) return fail(ND_ERR_ARG, "null argument");
  const size_t n = c->m.dec.size() * (size_t)c->cfg.max_steps;
  std::vector<unsigned long long> h(2 * n);
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipStreamSynchronize(c->es));
  HIPCHK(hipMemcpy(h.data(), c->kstamp, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  int rate_khz = 0;
  HIPCHK(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c->cfg.device));
  double sum = 0.0;
  int cnt = 0;
  for (size_t i = 0; i < n; ++i)
    if (h[2 * i] != ~0ull && h[2 * i + 1] >= h[2 * i]) {
      sum += (double)(h[2 * i + 1] - h[2 * i]);
      ++cnt;
    }
  *launches = cnt;
  *avg_us = cnt && rate_khz > 0 ? (float)(sum / cnt / rate_khz * 1e3) : 0.f;
  return ND_OK;
}

int nd_last_timing(nd_ctx* c, float* encode_ms, float* decode_ms) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  if (encode_ms) *encode_ms = c->t_enc;
  if (decode_ms) *decode_ms = c->t_dec;
  return ND_OK;
}

void nd_destroy(nd_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  if (c->es) (void)hipStreamSynchronize(c->es);
  drop_graphs(c);
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->h_alive) (void)hipHostFree(c->h_alive);
  for (hipEvent_t e : {c->ev_in, c->ev_out, c->ev_a, c->ev_b, c->ev_c})
    if (e) (void)hipEventDestroy(e);
  if (c->es) release_stream(c->cfg.device, c->es);  // synchronised above; recycled, not destroyed
  delete c;
}

int nd_bank_form(nd_ctx* c) { return c ? c->last_bank_form : 0; }
