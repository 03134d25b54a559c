// libnanodec_hip.so — the model side of a context: the weight registry, nd_load_weight, the attention
// rebalancing, the memory-bank derivations, nd_finalize and nd_share_weights.  Everything here fills
// struct Model (engine.hpp); calls only read it.
#include "engine.hpp"

static void add_slot(nd_ctx* c, const std::string& name, float* dst, std::vector<int64_t> shape, bool required = true,
                     int copy_rows = -1) {
  Slot s;
  s.dst = dst;
  s.shape = shape;
  s.numel = 1;
  for (auto d : shape) s.numel *= (size_t)d;
  s.required = required;
  s.copy_rows = copy_rows;
  c->slots[name] = s;
}

int build_registry(nd_ctx* c) {
  const int D = c->D, F = c->F, V = c->V;
  const auto& cfg = c->cfg;
  hipError_t e;
#define AL(ptr, n)                                          \
  if ((e = dalloc(c, &(ptr), (size_t)(n))) != hipSuccess) \
    return fail(ND_ERR_HIP, std::string("hipMalloc weights: ") + hipGetErrorString(e));
  if (cfg.encoder_type == ND_ENC_TRANSFORMER) {
    AL(c->m.enc_lin_w, D);
    AL(c->m.enc_lin_b, D);
    AL(c->m.enc_ln_g, D);
    AL(c->m.enc_ln_b, D);
    add_slot(c, "encoder.linear.weight", c->m.enc_lin_w, {D, 1});
    add_slot(c, "encoder.linear.bias", c->m.enc_lin_b, {D});
    add_slot(c, "encoder.layer_norm.weight", c->m.enc_ln_g, {D});
    add_slot(c, "encoder.layer_norm.bias", c->m.enc_ln_b, {D});
    c->m.enc.resize(cfg.enc_layers);
    for (int i = 0; i < cfg.enc_layers; ++i) {
      EncLayer& L = c->m.enc[i];
      AL(L.ln_g, D); AL(L.ln_b, D); AL(L.wqkv, 3 * D * D); AL(L.bqkv, 3 * D); AL(L.wo, D * D); AL(L.bo, D);
      AL(L.fln_g, D); AL(L.fln_b, D); AL(L.w1, (size_t)F * D); AL(L.b1, F); AL(L.w2, (size_t)D * F); AL(L.b2, D);
      AL(L.nwqkv, 3 * D * D); AL(L.nbqkv, 3 * D); AL(L.nw1, (size_t)F * D); AL(L.nb1, F);
      const std::string p = "encoder.transformer." + std::to_string(i);
      add_slot(c, p + ".layer_norm.weight", L.ln_g, {D});
      add_slot(c, p + ".layer_norm.bias", L.ln_b, {D});
      const char* qkv[3] = {"linear_query", "linear_keys", "linear_values"};
      for (int k = 0; k < 3; ++k) {
        add_slot(c, p + ".self_attn." + qkv[k] + ".weight", L.wqkv + (size_t)k * D * D, {D, D});
        add_slot(c, p + ".self_attn." + qkv[k] + ".bias", L.bqkv + k * D, {D});
      }
      add_slot(c, p + ".self_attn.final_linear.weight", L.wo, {D, D});
      add_slot(c, p + ".self_attn.final_linear.bias", L.bo, {D});
      add_slot(c, p + ".feed_forward.layer_norm.weight", L.fln_g, {D});
      add_slot(c, p + ".feed_forward.layer_norm.bias", L.fln_b, {D});
      add_slot(c, p + ".feed_forward.w_1.weight", L.w1, {F, D});
      add_slot(c, p + ".feed_forward.w_1.bias", L.b1, {F});
      add_slot(c, p + ".feed_forward.w_2.weight", L.w2, {D, F});
      add_slot(c, p + ".feed_forward.w_2.bias", L.b2, {D});
    }
  } else {
    const int Hh = c->H;
    c->m.nano.resize(cfg.enc_layers);
    for (int l = 0; l < cfg.enc_layers; ++l) {
      NanoLayer& L = c->m.nano[l];
      L.in = l == 0 ? 1 : 2 * Hh;
      AL(L.wih, (size_t)8 * Hh * L.in); AL(L.bih, 8 * Hh); AL(L.bhh, 8 * Hh); AL(L.whh, (size_t)8 * Hh * Hh);
      AL(L.bn_g, 2 * Hh); AL(L.bn_b, 2 * Hh); AL(L.bn_rm, 2 * Hh); AL(L.bn_rv, 2 * Hh);
      AL(L.bsum, 8 * Hh); AL(L.bn_scale, 2 * Hh); AL(L.bn_shift, 2 * Hh);
      const std::string p = "encoder.rnn_" + std::to_string(l);
      const char* sfx[2] = {"", "_reverse"};
      for (int d = 0; d < 2; ++d) {
        add_slot(c, p + ".weight_ih_l0" + sfx[d], L.wih + (size_t)d * 4 * Hh * L.in, {4 * Hh, L.in});
        add_slot(c, p + ".weight_hh_l0" + sfx[d], L.whh + (size_t)d * 4 * Hh * Hh, {4 * Hh, Hh});
        add_slot(c, p + ".bias_ih_l0" + sfx[d], L.bih + d * 4 * Hh, {4 * Hh});
        add_slot(c, p + ".bias_hh_l0" + sfx[d], L.bhh + d * 4 * Hh, {4 * Hh});
      }
      const std::string b = "encoder.batchnorm_" + std::to_string(l);
      add_slot(c, b + ".weight", L.bn_g, {2 * Hh});
      add_slot(c, b + ".bias", L.bn_b, {2 * Hh});
      add_slot(c, b + ".running_mean", L.bn_rm, {2 * Hh});
      add_slot(c, b + ".running_var", L.bn_rv, {2 * Hh});
    }
    AL(c->m.nano_W, (size_t)D * 2 * Hh);
    add_slot(c, "encoder.W.weight", c->m.nano_W, {D, 2 * Hh});
  }
  c->m.dec.resize(cfg.dec_layers);
  AL(c->m.ctxkv_w, (size_t)cfg.dec_layers * 2 * D * D);
  AL(c->m.ctxkv_b, (size_t)cfg.dec_layers * 2 * D);
  if (cfg.encoder_type == ND_ENC_TRANSFORMER) {
    AL(c->m.nctxkv_w, (size_t)cfg.dec_layers * 2 * D * D);
    AL(c->m.nctxkv_b, (size_t)cfg.dec_layers * 2 * D);
  }
  for (int i = 0; i < cfg.dec_layers; ++i) {
    DecLayer& L = c->m.dec[i];
    AL(L.ln1_g, D); AL(L.ln1_b, D); AL(L.wqkv, 3 * D * D); AL(L.bqkv, 3 * D); AL(L.wo, D * D); AL(L.bo, D);
    AL(L.ln2_g, D); AL(L.ln2_b, D); AL(L.cwq, D * D); AL(L.cbq, D); AL(L.cwo, D * D); AL(L.cbo, D);
    AL(L.fln_g, D); AL(L.fln_b, D); AL(L.w1, (size_t)F * D); AL(L.b1, F); AL(L.w2, (size_t)D * F); AL(L.b2, D);
    AL(L.nwqkv, 3 * D * D); AL(L.nbqkv, 3 * D); AL(L.ncwq, D * D); AL(L.ncbq, D); AL(L.nw1, (size_t)F * D);
    AL(L.nb1, F);
    AL(L.pwqkv, 3 * D * D); AL(L.pwo, D * D); AL(L.pcwq, D * D); AL(L.pcwo, D * D); AL(L.pw1, (size_t)F * D);
    AL(L.pw2, (size_t)D * F);
    AL(L.pwqk, (size_t)ND_H * D * D); AL(L.bqk, ND_H * D); AL(L.pwvo, (size_t)D * ND_H * D); AL(L.bvo, D);
    const std::string p = "decoder.transformer_layers." + std::to_string(i);
    add_slot(c, p + ".layer_norm_1.weight", L.ln1_g, {D});
    add_slot(c, p + ".layer_norm_1.bias", L.ln1_b, {D});
    add_slot(c, p + ".layer_norm_2.weight", L.ln2_g, {D});
    add_slot(c, p + ".layer_norm_2.bias", L.ln2_b, {D});
    if (cfg.self_attn_type == ND_SELF_AVERAGE) {
      AL(L.aln_g, D); AL(L.aln_b, D); AL(L.aw1, D * D); AL(L.ab1, D); AL(L.aw2, D * D); AL(L.ab2, D);
      AL(L.gw, 4 * D * D); AL(L.gb, 2 * D);
      AL(L.naw1, D * D); AL(L.nab1, D); AL(L.paw1, D * D); AL(L.paw2, D * D); AL(L.pgwx, 2 * D * D);
      AL(L.pgwa, 2 * D * D);
      const std::string a = p + ".self_attn.";
      add_slot(c, a + "average_layer.layer_norm.weight", L.aln_g, {D});
      add_slot(c, a + "average_layer.layer_norm.bias", L.aln_b, {D});
      add_slot(c, a + "average_layer.w_1.weight", L.aw1, {D, D});
      add_slot(c, a + "average_layer.w_1.bias", L.ab1, {D});
      add_slot(c, a + "average_layer.w_2.weight", L.aw2, {D, D});
      add_slot(c, a + "average_layer.w_2.bias", L.ab2, {D});
      add_slot(c, a + "gating_layer.weight", L.gw, {2 * D, 2 * D});
      add_slot(c, a + "gating_layer.bias", L.gb, {2 * D});
    } else {
      const char* qkv[3] = {"linear_query", "linear_keys", "linear_values"};
      for (int k = 0; k < 3; ++k) {
        add_slot(c, p + ".self_attn." + qkv[k] + ".weight", L.wqkv + (size_t)k * D * D, {D, D});
        add_slot(c, p + ".self_attn." + qkv[k] + ".bias", L.bqkv + k * D, {D});
      }
      add_slot(c, p + ".self_attn.final_linear.weight", L.wo, {D, D});
      add_slot(c, p + ".self_attn.final_linear.bias", L.bo, {D});
    }
    add_slot(c, p + ".context_attn.linear_query.weight", L.cwq, {D, D});
    add_slot(c, p + ".context_attn.linear_query.bias", L.cbq, {D});
    add_slot(c, p + ".context_attn.linear_keys.weight", c->m.ctxkv_w + (size_t)(2 * i) * D * D, {D, D});
    add_slot(c, p + ".context_attn.linear_keys.bias", c->m.ctxkv_b + (2 * i) * D, {D});
    add_slot(c, p + ".context_attn.linear_values.weight", c->m.ctxkv_w + (size_t)(2 * i + 1) * D * D, {D, D});
    add_slot(c, p + ".context_attn.linear_values.bias", c->m.ctxkv_b + (2 * i + 1) * D, {D});
    add_slot(c, p + ".context_attn.final_linear.weight", L.cwo, {D, D});
    add_slot(c, p + ".context_attn.final_linear.bias", L.cbo, {D});
    add_slot(c, p + ".feed_forward.layer_norm.weight", L.fln_g, {D});
    add_slot(c, p + ".feed_forward.layer_norm.bias", L.fln_b, {D});
    add_slot(c, p + ".feed_forward.w_1.weight", L.w1, {F, D});
    add_slot(c, p + ".feed_forward.w_1.bias", L.b1, {F});
    add_slot(c, p + ".feed_forward.w_2.weight", L.w2, {D, F});
    add_slot(c, p + ".feed_forward.w_2.bias", L.b2, {D});
  }
  AL(c->m.emb, (size_t)V * D);
  add_slot(c, "decoder.embeddings.make_embedding.emb_luts.0.weight", c->m.emb, {V, D});
  if (cfg.position_encoding) {
    AL(c->m.pe, (size_t)cfg.max_steps * D);
    add_slot(c, "decoder.embeddings.make_embedding.pe.pe", c->m.pe, {-1, 1, D}, true, cfg.max_steps);
  }
  AL(c->m.dec_ln_g, D);
  AL(c->m.dec_ln_b, D);
  add_slot(c, "decoder.layer_norm.weight", c->m.dec_ln_g, {D});
  add_slot(c, "decoder.layer_norm.bias", c->m.dec_ln_b, {D});
  AL(c->m.gen_w, (size_t)V * D);
  AL(c->m.gen_b, V);
  add_slot(c, "generator.0.weight", c->m.gen_w, {V, D});
  add_slot(c, "generator.0.bias", c->m.gen_b, {V});
#undef AL
  return ND_OK;
}

int nd_load_weight(nd_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!c || !name || !host || (!shape && ndim > 0)) return fail(ND_ERR_ARG, "null argument");
  if (c->shares) return fail(ND_ERR_STATE, "nd_load_weight: the context reads another context's weights");
  const std::string n(name);
  auto it = c->slots.find(n);
  if (it == c->slots.end()) {
    auto ends = [&](const char* sfx) {
      const size_t k = strlen(sfx);
      return n.size() >= k && n.compare(n.size() - k, k, sfx) == 0;
    };
    if (ends(".mask") || ends("num_batches_tracked")) return ND_OK;  // buffers the engine does not use
    if (!c->cfg.position_encoding && n == "decoder.embeddings.make_embedding.pe.pe") return ND_OK;
    return fail(ND_ERR_WEIGHT, "unknown weight '" + n + "'");
  }
  Slot& s = it->second;
  if ((size_t)ndim != s.shape.size()) return fail(ND_ERR_WEIGHT, "rank mismatch for '" + n + "'");
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) {
    if (s.shape[i] >= 0 && shape[i] != s.shape[i]) return fail(ND_ERR_WEIGHT, "shape mismatch for '" + n + "'");
    numel *= (size_t)shape[i];
  }
  size_t copy = numel;
  if (s.copy_rows >= 0) {
    if (shape[0] < s.copy_rows) return fail(ND_ERR_WEIGHT, "'" + n + "' has fewer rows than max_steps");
    copy = (size_t)s.copy_rows * (numel / (size_t)shape[0]);
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  auto rs = c->rescale.find(s.dst);
  if (rs != c->rescale.end()) {  // a weight the context already rebalanced: the same exact scales
    const auto& R = rs->second;
    const size_t cols = ndim >= 2 ? (size_t)shape[ndim - 1] : 1;
    std::vector<float> tmp(host, host + copy);
    for (size_t e = 0; e < copy; ++e) tmp[e] *= R.s[R.cols ? e % cols : e / cols];
    HIPCHK(hipMemcpy(s.dst, tmp.data(), copy * sizeof(float), hipMemcpyHostToDevice));
  } else {
    HIPCHK(hipMemcpy(s.dst, host, copy * sizeof(float), hipMemcpyHostToDevice));
  }
  s.loaded = true;
  c->finalized = false;
  return ND_OK;
}

// P16 step weight (fp32, for the fp32 kernels) and its split-fp16 P16H image
// (gemm.hip H3), registered under the P16 pointer for G::h3
static hipError_t pack_step_weight(nd_ctx* c, const float* src, int ld, float* dst, int rows, int cols) {
  hipError_t e = nd::launch_pack_p16(src, ld, dst, rows, cols, c->es);
  if (e != hipSuccess) return e;
  uint16_t* h = nullptr;
  auto it = c->m.split.find(dst);
  if (it != c->m.split.end()) h = it->second.first;  // finalize called again: refresh in place
  // hi and lo halves: two per element
  if (!h && (e = dalloc(c, &h, (size_t)2 * rows * cols)) != hipSuccess) return e;
  float sc = 1.f;
  if ((e = nd::launch_pack_p16h(src, ld, rows, cols, h, &sc, c->es)) != hipSuccess) return e;
  c->m.split[dst] = {h, sc};
  // and the row-major image for the LDS-tiled kernel (many rows)
  uint16_t* hr = nullptr;
  auto jt = c->m.split_rm.find(dst);
  if (jt != c->m.split_rm.end()) hr = jt->second.first;
  if (!hr && (e = dalloc(c, &hr, (size_t)2 * rows * cols)) != hipSuccess) return e;
  if ((e = nd::launch_split_weight(src, ld, rows, cols, hr, &sc, c->es)) != hipSuccess) return e;
  c->m.split_rm[dst] = {hr, sc};
  return hipSuccess;
}

// Per-dimension power-of-two rebalancing of the decoder's attentions (self
// and context, onmt/modules/multi_headed_attn.py:124-177).  The beam path
// stores keys and values as 24-bit integers with one scale per (key, head)
// (the context K/V image, the self-attention history), so a dimension far
// larger than the rest of its head -- an "outlier dimension", common in
// trained transformers -- would cost the head's other dimensions that many
// bits.  Scores q.k and the context W_o v are unchanged when key dimension j
// is divided by c_j and query dimension j multiplied by it (value dimension
// j divided, output column j multiplied), so with c_j a power of two the
// model's function is unchanged in exact arithmetic and in fp32 alike.  c_j =
// 2^clamp(floor(log2(a_j / median of a over j's head)), 0, 12), a_j the
// predicted magnitude of projection row j over its input (a LayerNorm output
// y = n g + b: mean b, variance g^2; the NanoEncoder's memory: 0, 1):
// sqrt(sum_i W_ji^2 g_i^2) + |bias_j + sum_i W_ji b_i|.  Applied in place to
// the loaded weights once (nd_finalize); a weight loaded into the context
// afterwards gets the same scales (nd_load_weight).
static void rebalance_scales(const std::vector<float>& W, const std::vector<float>& b, const float* mu,
                             const float* var, int D, std::vector<float>& c) {
  std::vector<double> a(D);
  for (int j = 0; j < D; ++j) {
    double v = 0.0, m = b[j];
    for (int i = 0; i < D; ++i) {
      const double w = W[(size_t)j * D + i];
      v += w * w * (var ? (double)var[i] : 1.0);
      m += mu ? w * mu[i] : 0.0;
    }
    a[j] = std::sqrt(v) + std::fabs(m);
  }
  c.assign(D, 1.f);
  for (int h = 0; h < ND_H; ++h) {
    std::vector<double> hd(a.begin() + h * ND_DH, a.begin() + (h + 1) * ND_DH);
    std::nth_element(hd.begin(), hd.begin() + ND_DH / 2, hd.end());
    const double med = hd[ND_DH / 2];
    for (int j = h * ND_DH; j < (h + 1) * ND_DH; ++j) {
      int k = 0;
      if (med > 0 && a[j] > 0 && std::isfinite(a[j])) k = (int)std::floor(std::log2(a[j] / med));
      c[j] = std::ldexp(1.f, std::min(std::max(k, 0), 12));
    }
  }
}

static int rebalance_attention(nd_ctx* c) {
  if (c->rebalanced) return ND_OK;
  const int D = c->D;
  auto down = [&](const float* d, size_t n, std::vector<float>& h) {
    h.resize(n);
    return hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost);
  };
  // scale rows (or columns) of a D x D buffer / a D vector by f(c_j), upload, record the scales
  auto apply = [&](float* dst, std::vector<float>& h, const std::vector<float>& cs, bool inv, bool cols,
                   size_t rows) -> hipError_t {
    nd_ctx::Rescale R;
    R.cols = cols;
    R.s.resize(cs.size());
    for (size_t j = 0; j < cs.size(); ++j) R.s[j] = inv ? 1.f / cs[j] : cs[j];
    const size_t ncol = h.size() / rows;
    for (size_t e = 0; e < h.size(); ++e) h[e] *= R.s[cols ? e % ncol : e / ncol];
    c->rescale[dst] = R;
    return hipMemcpy(dst, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  };
  std::vector<float> g, bb, Wq, bq, Wk, bk, Wv, bv, Wo, ck, cv;
  std::vector<float> mg, mb;  // the memory's LN affine (transformer encoder)
  const bool tf = c->cfg.encoder_type == ND_ENC_TRANSFORMER;
  if (tf) {
    HIPCHK(down(c->m.enc_ln_g, D, mg));
    HIPCHK(down(c->m.enc_ln_b, D, mb));
    for (auto& x : mg) x *= x;  // variance g^2
  }
  for (size_t i = 0; i < c->m.dec.size(); ++i) {
    DecLayer& L = c->m.dec[i];
    if (c->cfg.self_attn_type != ND_SELF_AVERAGE) {
      HIPCHK(down(L.ln1_g, D, g));
      HIPCHK(down(L.ln1_b, D, bb));
      for (auto& x : g) x *= x;
      HIPCHK(down(L.wqkv, (size_t)D * D, Wq));
      HIPCHK(down(L.bqkv, D, bq));
      HIPCHK(down(L.wqkv + (size_t)D * D, (size_t)D * D, Wk));
      HIPCHK(down(L.bqkv + D, D, bk));
      HIPCHK(down(L.wqkv + (size_t)2 * D * D, (size_t)D * D, Wv));
      HIPCHK(down(L.bqkv + 2 * D, D, bv));
      HIPCHK(down(L.wo, (size_t)D * D, Wo));
      rebalance_scales(Wk, bk, bb.data(), g.data(), D, ck);
      rebalance_scales(Wv, bv, bb.data(), g.data(), D, cv);
      HIPCHK(apply(L.wqkv, Wq, ck, false, false, D));
      HIPCHK(apply(L.bqkv, bq, ck, false, false, D));
      HIPCHK(apply(L.wqkv + (size_t)D * D, Wk, ck, true, false, D));
      HIPCHK(apply(L.bqkv + D, bk, ck, true, false, D));
      HIPCHK(apply(L.wqkv + (size_t)2 * D * D, Wv, cv, true, false, D));
      HIPCHK(apply(L.bqkv + 2 * D, bv, cv, true, false, D));
      HIPCHK(apply(L.wo, Wo, cv, false, true, D));
    }
    float* wk = c->m.ctxkv_w + (size_t)(2 * i) * D * D;
    float* wv = c->m.ctxkv_w + (size_t)(2 * i + 1) * D * D;
    float* bk_ = c->m.ctxkv_b + (size_t)(2 * i) * D;
    float* bv_ = c->m.ctxkv_b + (size_t)(2 * i + 1) * D;
    HIPCHK(down(L.cwq, (size_t)D * D, Wq));
    HIPCHK(down(L.cbq, D, bq));
    HIPCHK(down(wk, (size_t)D * D, Wk));
    HIPCHK(down(bk_, D, bk));
    HIPCHK(down(wv, (size_t)D * D, Wv));
    HIPCHK(down(bv_, D, bv));
    HIPCHK(down(L.cwo, (size_t)D * D, Wo));
    rebalance_scales(Wk, bk, tf ? mb.data() : nullptr, tf ? mg.data() : nullptr, D, ck);
    rebalance_scales(Wv, bv, tf ? mb.data() : nullptr, tf ? mg.data() : nullptr, D, cv);
    HIPCHK(apply(L.cwq, Wq, ck, false, false, D));
    HIPCHK(apply(L.cbq, bq, ck, false, false, D));
    HIPCHK(apply(wk, Wk, ck, true, false, D));
    HIPCHK(apply(bk_, bk, ck, true, false, D));
    HIPCHK(apply(wv, Wv, cv, true, false, D));
    HIPCHK(apply(bv_, bv, cv, true, false, D));
    HIPCHK(apply(L.cwo, Wo, cv, false, true, D));
  }
  c->rebalanced = true;
  return ND_OK;
}

// Per-dimension power-of-two scales of the memory bank (transformer encoder).
// The bank holds m_i / c_i with m = LN(x) g + b (encoder/transformer.py:127):
// a dimension whose LN affine makes it far larger than the rest (an "outlier
// dimension", common in trained transformers) would otherwise set every row's
// 24-bit scale (bank8.hip: one scale per key row) and cost the other
// dimensions that many bits.  c_i = 2^k_i, k_i = clamp(floor(log2(a_i /
// median a)), 0, 12), a_i = 3 |g_i| + |b_i| (a LayerNorm'd value lies mostly
// within +-3); c_i is folded back exactly into W_qk's rows and W_vo's
// columns (derive_memory_bank_weights), so scores and context vectors are
// unchanged in exact arithmetic.  The NanoEncoder's bank keeps c = 1.
static int derive_bank_dim_scales(nd_ctx* c) {
  const int D = c->D;
  c->m.bank_dim_scale.assign(D, 1.f);
  if (c->cfg.encoder_type != ND_ENC_TRANSFORMER) return ND_OK;
  std::vector<float> g(D), b(D);
  HIPCHK(hipMemcpy(g.data(), c->m.enc_ln_g, D * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(b.data(), c->m.enc_ln_b, D * 4, hipMemcpyDeviceToHost));
  std::vector<double> a(D);
  for (int i = 0; i < D; ++i) a[i] = 3.0 * std::fabs((double)g[i]) + std::fabs((double)b[i]);
  std::vector<double> srt(a);
  std::nth_element(srt.begin(), srt.begin() + D / 2, srt.end());
  const double med = srt[D / 2];
  for (int i = 0; i < D; ++i) {
    int k = 0;
    if (med > 0 && a[i] > 0 && std::isfinite(a[i])) k = (int)std::floor(std::log2(a[i] / med));
    k = std::min(std::max(k, 0), 12);
    c->m.bank_dim_scale[i] = std::ldexp(1.f, k);
    g[i] = std::ldexp(g[i], -k);
    b[i] = std::ldexp(b[i], -k);
  }
  if (!c->m.bank_ln_g && dalloc(c, &c->m.bank_ln_g, D) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
  if (!c->m.bank_ln_b && dalloc(c, &c->m.bank_ln_b, D) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
  HIPCHK(hipMemcpy(c->m.bank_ln_g, g.data(), D * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->m.bank_ln_b, b.data(), D * 4, hipMemcpyHostToDevice));
  return ND_OK;
}

// Memory-bank form of the context attention (attention.hip): per decoder
// layer, in f64 on the host from the reference weights,
//   W_qk[h*256+i][k] = sum_a W_k[32h+a][i] W_q'[32h+a][k] / sqrt(32)
//   b_qk[h*256+i]    = sum_a W_k[32h+a][i] b_q'[32h+a]     / sqrt(32)
//   W_vo[n][h*256+i] = sum_a W_o[n][32h+a] W_v[32h+a][i]
//   b_vo[n]          = W_o[n] . b_v + b_o[n]
// with W_q' = W_q diag(ln2_g), b_q' = W_q ln2_b + b_q (layer_norm_2 folded).
// q_h . b_k,h is constant over keys and drops out of the softmax exactly.
// Row h*256+i of W_qk / b_qk and column h*256+i of W_vo carry the bank's
// per-dimension scale c_i (derive_bank_dim_scales; powers of two: exact).
static int derive_memory_bank_weights(nd_ctx* c) {
  const int D = c->D, H = ND_H, DH = ND_DH, Ld = (int)c->m.dec.size();
  auto down = [&](const float* d, size_t n, std::vector<float>& h) {
    h.resize(n);
    return hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost);
  };
  float* scratch = nullptr;
  HIPCHK(hipMalloc(&scratch, (size_t)H * D * D * sizeof(float)));
  std::vector<float> Wq, bq, g2, b2, Wk, Wv, bv, Wo, bo;
  std::vector<float> wqk((size_t)H * D * D), bqk((size_t)H * D), wvo((size_t)D * H * D), bvo(D);
  int rc = ND_OK;
  for (int i = 0; i < Ld && rc == ND_OK; ++i) {
    DecLayer& L = c->m.dec[i];
    hipError_t e = hipSuccess;
    if ((e = down(L.cwq, (size_t)D * D, Wq)) != hipSuccess || (e = down(L.cbq, D, bq)) != hipSuccess ||
        (e = down(L.ln2_g, D, g2)) != hipSuccess || (e = down(L.ln2_b, D, b2)) != hipSuccess ||
        (e = down(c->m.ctxkv_w + (size_t)(2 * i) * D * D, (size_t)D * D, Wk)) != hipSuccess ||
        (e = down(c->m.ctxkv_w + (size_t)(2 * i + 1) * D * D, (size_t)D * D, Wv)) != hipSuccess ||
        (e = down(c->m.ctxkv_b + (size_t)(2 * i + 1) * D, D, bv)) != hipSuccess ||
        (e = down(L.cwo, (size_t)D * D, Wo)) != hipSuccess || (e = down(L.cbo, D, bo)) != hipSuccess) {
      rc = fail(ND_ERR_HIP, std::string("memory-bank weights: ") + hipGetErrorString(e));
      break;
    }
    const double inv = 1.0 / std::sqrt((double)DH);
    std::vector<double> wq2((size_t)D * D), bq2(D);
    for (int a = 0; a < D; ++a) {
      double sb = bq[a];
      for (int k = 0; k < D; ++k) {
        wq2[(size_t)a * D + k] = (double)Wq[(size_t)a * D + k] * g2[k];
        sb += (double)Wq[(size_t)a * D + k] * b2[k];
      }
      bq2[a] = sb;
    }
    std::vector<double> row(D);
    for (int h = 0; h < H; ++h)
      for (int ii = 0; ii < D; ++ii) {
        std::fill(row.begin(), row.end(), 0.0);
        double sb = 0.0;
        for (int a = 0; a < DH; ++a) {
          const double wk = Wk[(size_t)(h * DH + a) * D + ii];
          const double* wr = &wq2[(size_t)(h * DH + a) * D];
          for (int k = 0; k < D; ++k) row[k] += wk * wr[k];
          sb += wk * bq2[h * DH + a];
        }
        const double ci = c->m.bank_dim_scale[ii];
        for (int k = 0; k < D; ++k) wqk[((size_t)h * D + ii) * D + k] = (float)(row[k] * inv * ci);
        bqk[(size_t)h * D + ii] = (float)(sb * inv * ci);
      }
    for (int n = 0; n < D; ++n) {
      double sb = bo[n];
      for (int j = 0; j < D; ++j) sb += (double)Wo[(size_t)n * D + j] * bv[j];
      bvo[n] = (float)sb;
      for (int h = 0; h < H; ++h) {
        std::fill(row.begin(), row.end(), 0.0);
        for (int a = 0; a < DH; ++a) {
          const double wo = Wo[(size_t)n * D + h * DH + a];
          const float* vr = &Wv[(size_t)(h * DH + a) * D];
          for (int ii = 0; ii < D; ++ii) row[ii] += wo * vr[ii];
        }
        for (int ii = 0; ii < D; ++ii) wvo[(size_t)n * H * D + h * D + ii] = (float)(row[ii] * c->m.bank_dim_scale[ii]);
      }
    }
    if ((e = hipMemcpy(scratch, wqk.data(), wqk.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = pack_step_weight(c, scratch, D, L.pwqk, H * D, D)) != hipSuccess ||
        (e = hipStreamSynchronize(c->es)) != hipSuccess ||
        (e = hipMemcpy(scratch, wvo.data(), wvo.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = pack_step_weight(c, scratch, H * D, L.pwvo, D, H * D)) != hipSuccess ||
        (e = hipStreamSynchronize(c->es)) != hipSuccess ||
        (e = hipMemcpy(L.bqk, bqk.data(), bqk.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(L.bvo, bvo.data(), bvo.size() * 4, hipMemcpyHostToDevice)) != hipSuccess)
      rc = fail(ND_ERR_HIP, std::string("memory-bank weights: ") + hipGetErrorString(e));
  }
  (void)hipFree(scratch);
  return rc;
}

// Decoder layer 0's QKV table (Model.qtab): QKV0[s][v] = LN(emb[v] (* 16 + pe[s])) W_qkv + b for every
// step s < max_steps and token v, the layer-0 projection of every input a step can see, through the same
// GEMM the step would run (decoder/transformer.py:76-78, the embedding as
// onmt/modules/embeddings.py:189-207): once on the split-fp16 weight image, once in exact fp32.  Row-major:
// the self-attention reads whole rows (QkvRows.rm).  Every buffer, the input rows and their statistics
// included, is allocated once and kept: freeing device memory here (hipMalloc / hipFree of the two scratch
// buffers) made a split-K context's third and later graph launches return wrong tokens on MI355X.
static int build_qkv_tables(nd_ctx* c) {
  if (c->cfg.self_attn_type == ND_SELF_AVERAGE) return ND_OK;
  const int D = c->D, S = c->cfg.max_steps;
  const size_t rows = ((size_t)S * c->V + 15) / 16 * 16;
  Model& m = c->m;
  for (auto& t : m.qtab)
    if (!t && dalloc(c, &t, rows * 3 * D) != hipSuccess) return fail(ND_ERR_HIP, "hipMalloc layer-0 QKV table");
  if (!m.qtab_x && dalloc(c, &m.qtab_x, rows * D) != hipSuccess) return fail(ND_ERR_HIP, "hipMalloc layer-0 QKV table");
  if (!m.qtab_part && dalloc(c, &m.qtab_part, rows * ND_PART_LD * 2) != hipSuccess)
    return fail(ND_ERR_HIP, "hipMalloc layer-0 QKV table");
  m.qtab_steps = S;
  const bool exact = c->exact;
  hipError_t e = hipMemsetAsync(m.qtab_x, 0, rows * D * sizeof(float), c->es);
  if (e == hipSuccess) e = hipMemsetAsync(m.qtab_part, 0, rows * ND_PART_LD * 2 * sizeof(float), c->es);
  if (e == hipSuccess)
    e = nd::launch_dec_embed_table(m.emb, c->cfg.position_encoding ? m.pe : nullptr, c->V, S, m.qtab_x, m.qtab_part,
                                   (int)rows, c->es);
  const DecLayer& L = m.dec[0];
  for (int ex = 0; ex < 2 && e == hipSuccess; ++ex) {
    c->exact = ex != 0;  // G::h3 picks the weight image by it
    e = G(m.qtab_x, D, L.pwqkv, 3 * D, D, L.nbqkv, m.qtab[ex], 3 * D, (int)rows)
            .p16()
            .h3(c)
            .ln(m.qtab_part, 1)
            .c_rowmajor(true)
            .run(c->es);
  }
  c->exact = exact;
  if (e == hipSuccess) e = hipStreamSynchronize(c->es);
  if (e != hipSuccess) return fail(ND_ERR_HIP, std::string("layer-0 QKV table: ") + hipGetErrorString(e));
  return ND_OK;
}

int nd_finalize(nd_ctx* c) {
  if (!c) return fail(ND_ERR_ARG, "null ctx");
  std::string missing;
  for (auto& kv : c->slots)
    if (kv.second.required && !kv.second.loaded) missing += (missing.empty() ? "" : ", ") + kv.first;
  if (!missing.empty()) return fail(ND_ERR_WEIGHT, "missing weights: " + missing);
  HIPCHK(hipSetDevice(c->cfg.device));
  if (int rc = rebalance_attention(c)) return rc;
  if (c->cfg.encoder_type == ND_ENC_NANO) {
    // derived: b_ih + b_hh per gate; eval BatchNorm as scale/shift
    const int Hh = c->H;
    for (auto& L : c->m.nano) {
      std::vector<float> bih(8 * Hh), bhh(8 * Hh), g(2 * Hh), b(2 * Hh), rm(2 * Hh), rv(2 * Hh);
      HIPCHK(hipMemcpy(bih.data(), L.bih, bih.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(bhh.data(), L.bhh, bhh.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(g.data(), L.bn_g, g.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(b.data(), L.bn_b, b.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(rm.data(), L.bn_rm, rm.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(rv.data(), L.bn_rv, rv.size() * 4, hipMemcpyDeviceToHost));
      std::vector<float> bs(8 * Hh), sc(2 * Hh), sh(2 * Hh);
      for (int i = 0; i < 8 * Hh; ++i) bs[i] = bih[i] + bhh[i];
      for (int i = 0; i < 2 * Hh; ++i) {
        sc[i] = (float)(1.0 / std::sqrt((double)rv[i] + 1e-5)) * g[i];
        sh[i] = b[i] - rm[i] * sc[i];
      }
      HIPCHK(hipMemcpy(L.bsum, bs.data(), bs.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(L.bn_scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(L.bn_shift, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
    }
  }
  // LayerNorm affines folded into the Linear that consumes them
  {
    const int D = c->D, F = c->F;
    auto fold = [&](const float* W, const float* b, const float* g, const float* be, float* Wo, float* bo, int N,
                    int K) { return nd::launch_fold_layernorm(W, b, g, be, Wo, bo, N, K, c->es); };
    for (auto& L : c->m.enc) {
      HIPCHK(fold(L.wqkv, L.bqkv, L.ln_g, L.ln_b, L.nwqkv, L.nbqkv, 3 * D, D));
      HIPCHK(fold(L.w1, L.b1, L.fln_g, L.fln_b, L.nw1, L.nb1, F, D));
    }
    if (c->cfg.encoder_type == ND_ENC_TRANSFORMER && !c->m.enc.empty()) {
      if (!c->m.eq_ac && dalloc(c, &c->m.eq_ac, (size_t)6 * D) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
      if (!c->m.eq_scal && dalloc(c, &c->m.eq_scal, 4) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
      if (!c->m.eq_coef && dalloc(c, &c->m.eq_coef, (size_t)ND_H * 6) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
      // a | c, the means, s0 and the per-head coefficients of the closed form (attention.hip)
      HIPCHK(nd::prepare_embed_qkv(c->m.enc_lin_w, c->m.enc_lin_b, c->m.enc[0].nwqkv, c->m.enc[0].nbqkv, c->m.eq_ac,
                                   c->m.eq_scal, c->m.eq_coef, &c->m.eq, c->es));
    }
    if (c->m.nctxkv_w)
      HIPCHK(fold(c->m.ctxkv_w, c->m.ctxkv_b, c->m.enc_ln_g, c->m.enc_ln_b, c->m.nctxkv_w, c->m.nctxkv_b,
                  (int)c->m.dec.size() * 2 * D, D));
    for (auto& L : c->m.dec) {
      if (c->cfg.self_attn_type == ND_SELF_AVERAGE) {
        HIPCHK(fold(L.aw1, L.ab1, L.aln_g, L.aln_b, L.naw1, L.nab1, D, D));
        HIPCHK(pack_step_weight(c, L.naw1, D, L.paw1, D, D));
        HIPCHK(pack_step_weight(c, L.aw2, D, L.paw2, D, D));
        HIPCHK(pack_step_weight(c, L.gw, 2 * D, L.pgwx, 2 * D, D));      // gate columns of xn
        HIPCHK(pack_step_weight(c, L.gw + D, 2 * D, L.pgwa, 2 * D, D));  // gate columns of a
      } else {
        HIPCHK(fold(L.wqkv, L.bqkv, L.ln1_g, L.ln1_b, L.nwqkv, L.nbqkv, 3 * D, D));
        HIPCHK(pack_step_weight(c, L.nwqkv, D, L.pwqkv, 3 * D, D));
        HIPCHK(pack_step_weight(c, L.wo, D, L.pwo, D, D));
      }
      HIPCHK(fold(L.cwq, L.cbq, L.ln2_g, L.ln2_b, L.ncwq, L.ncbq, D, D));
      HIPCHK(fold(L.w1, L.b1, L.fln_g, L.fln_b, L.nw1, L.nb1, F, D));
      HIPCHK(pack_step_weight(c, L.ncwq, D, L.pcwq, D, D));
      HIPCHK(pack_step_weight(c, L.cwo, D, L.pcwo, D, D));
      HIPCHK(pack_step_weight(c, L.nw1, D, L.pw1, F, D));
      HIPCHK(pack_step_weight(c, L.w2, F, L.pw2, D, F));
    }
    HIPCHK(hipStreamSynchronize(c->es));
  }
  {
    // split-fp16 images of the encoder-side row-major GEMM weights
    // (gemm.hip H3); exact fp32 (nd_set_exact_fp32) keeps the fp32 kernels
    const int D = c->D, F = c->F, L2 = (int)c->m.dec.size() * 2 * D;
    hipError_t e_ = hipSuccess;
    auto mk = [&](const float* W, int N, int K) -> hipError_t {
      uint16_t* h = nullptr;
      float sc = 1.f;
      auto it = c->m.split.find(W);
      if (it != c->m.split.end()) h = it->second.first;  // finalize called again: refresh in place
      hipError_t e = h ? hipSuccess : dalloc(c, &h, (size_t)2 * N * K);
      if (e == hipSuccess) e = nd::launch_split_weight(W, K, N, K, h, &sc, c->es);
      if (e == hipSuccess) c->m.split[W] = {h, sc};
      return e;
    };
    for (auto& L : c->m.enc) {
      HIPCHK(mk(L.nwqkv, 3 * D, D));
      HIPCHK(mk(L.wo, D, D));
      HIPCHK(mk(L.nw1, F, D));
      HIPCHK(mk(L.w2, D, F));
      if (F % 32 == 0 && F <= 2048) {  // the fused FFN block's weight images
        if (!L.w1h && (e_ = dalloc(c, &L.w1h, (size_t)2 * F * D)) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
        if (!L.w2h && (e_ = dalloc(c, &L.w2h, (size_t)2 * F * D)) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
        HIPCHK(nd::launch_pack_p16h(L.nw1, D, F, D, L.w1h, &L.w1s, c->es));
        HIPCHK(nd::launch_pack_p16h(L.w2, F, D, F, L.w2h, &L.w2s, c->es));
        if (!L.woh && (e_ = dalloc(c, &L.woh, (size_t)2 * D * D)) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
        HIPCHK(nd::launch_pack_p16h(L.wo, D, D, D, L.woh, &L.wos, c->es));
        if (!L.qkvh && (e_ = dalloc(c, &L.qkvh, (size_t)2 * 3 * D * D)) != hipSuccess) return fail(ND_ERR_HIP, "alloc");
        HIPCHK(nd::launch_pack_p16h(L.nwqkv, D, 3 * D, D, L.qkvh, &L.qkvs, c->es));
      }
    }
    HIPCHK(mk(c->cfg.encoder_type == ND_ENC_TRANSFORMER ? c->m.nctxkv_w : c->m.ctxkv_w, L2, D));
    // teacher-forced scoring (engine.hip enqueue_score) runs the decoder's fp32 row-major weights over
    // B * L rows on the same GEMMs
    if (c->cfg.self_attn_type != ND_SELF_AVERAGE)
      for (auto& L : c->m.dec) {
        HIPCHK(mk(L.nwqkv, 3 * D, D));
        HIPCHK(mk(L.wo, D, D));
        HIPCHK(mk(L.ncwq, D, D));
        HIPCHK(mk(L.cwo, D, D));
        HIPCHK(mk(L.nw1, F, D));
        HIPCHK(mk(L.w2, D, F));
      }
    for (size_t l = 1; l < c->m.nano.size(); ++l) HIPCHK(mk(c->m.nano[l].wih, 8 * c->H, 2 * c->H));
    if (c->m.nano_W) HIPCHK(mk(c->m.nano_W, D, 2 * c->H));
    HIPCHK(hipStreamSynchronize(c->es));
  }
  {
    int rc = derive_bank_dim_scales(c);
    if (!rc) rc = derive_memory_bank_weights(c);
    if (!rc) rc = build_qkv_tables(c);
    if (rc) return rc;
  }
  drop_graphs(c);
  c->finalized = true;
  return ND_OK;
}

int nd_share_weights(nd_ctx* c, const nd_ctx* src) {
  if (!c || !src) return fail(ND_ERR_ARG, "null ctx");
  if (!src->finalized) return fail(ND_ERR_STATE, "nd_share_weights: the source context is not finalized");
  if (c == src || c->finalized) return fail(ND_ERR_STATE, "nd_share_weights: the context already holds weights");
  for (const auto& kv : c->slots)
    if (kv.second.loaded) return fail(ND_ERR_STATE, "nd_share_weights: weights were loaded into the context");
  const nd_config &a = c->cfg, &b = src->cfg;
  if (a.encoder_type != b.encoder_type || a.self_attn_type != b.self_attn_type || a.enc_layers != b.enc_layers ||
      a.dec_layers != b.dec_layers || a.d_model != b.d_model || a.heads != b.heads || a.d_ff != b.d_ff ||
      a.vocab != b.vocab || a.rnn_hidden != b.rnn_hidden || a.position_encoding != b.position_encoding ||
      a.pad_idx != b.pad_idx || a.bos_idx != b.bos_idx || a.eos_idx != b.eos_idx || a.device != b.device)
    return fail(ND_ERR_ARG, "nd_share_weights: the model configurations differ");
  // the position table and the layer-0 QKV table hold the source's max_steps steps
  if (a.max_steps > b.max_steps) return fail(ND_ERR_ARG, "nd_share_weights: max_steps exceeds the source context's");
  // every weight pointer and every image nd_finalize derived (struct Model; nothing in it is a workspace).
  // The context's own raw weight buffers from nd_create stay allocated and are never read (a few tens of MB
  // at d_model 256): the derived images -- the split-fp16 and P16 forms, the memory-bank products -- are
  // what sharing saves, and every lane reads one copy.
  c->m = src->m;
  drop_graphs(c);
  c->shares = true;
  c->finalized = true;
  return ND_OK;
}
