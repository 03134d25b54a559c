// libnanodec_hip.so — the op-level entry points (nd_op_*, nd_normalize_reads, nd_window_reads,
// nd_assemble_reads, nd_assemble_reads_q, nd_assemble_reads_m, nd_assemble_reads_p, nd_token_weights, nd_token_mod_weights, nd_token_positions, nd_align_seqs, nd_locate_segs, nd_align_fit, nd_align_fit_pos, nd_pileup_add, nd_pileup_call): launches on the caller's stream, with no context.
// The nd_op_* calls exist for the op-level tests.
#include "engine.hpp"

// an entry's status from its launcher's: "name: <the HIP error's text>" in nd_last_error
static int status(const char* name, hipError_t e, int code = ND_ERR_ARG) {
  return e == hipSuccess ? ND_OK : fail(code, std::string(name) + ": " + hipGetErrorString(e));
}
// the P16 GEMM entries also report the output's row partials
static int status_p16(const char* name, nd::GemmArgs g, int32_t* part_n_out, void* stream) {
  const int rc = status(name, nd::launch_gemm_p16(g, (hipStream_t)stream));
  if (rc == ND_OK && part_n_out) *part_n_out = g.part_n_out;
  return rc;
}

int nd_op_gemm(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M, int32_t N,
               int32_t K, int32_t norm, int32_t relu, void* stream) {
  nd::GemmArgs g{.A = A, .lda = K, .W = W, .ldw = K, .bias = bias, .R = R, .ldr = N, .C = C, .ldc = N,
                 .norm = norm != 0, .M = M, .N = N, .K = K, .relu = relu != 0};
  return status("gemm", nd::launch_gemm(g, (hipStream_t)stream));
}

int nd_op_split_weight(const float* W, int32_t N, int32_t K, uint16_t* Wh, float* wscale, void* stream) {
  return status("split_weight", nd::launch_split_weight(W, K, N, K, Wh, wscale, (hipStream_t)stream));
}

int nd_op_gemm_split(const float* A, const uint16_t* Wh, float wscale, const float* bias, const float* R, float* C,
                     int32_t M, int32_t N, int32_t K, int32_t norm, int32_t relu, void* stream) {
  if (!Wh) return fail(ND_ERR_ARG, "gemm_split: null Wh");
  nd::GemmArgs g{.A = A, .lda = K, .ldw = K, .bias = bias, .R = R, .ldr = R ? N : 0, .C = C, .ldc = N,
                 .norm = norm != 0, .M = M, .N = N, .K = K, .relu = relu != 0, .Wh = Wh, .wscale = wscale};
  return status("gemm_split", nd::launch_gemm(g, (hipStream_t)stream));
}

int nd_op_gemm_split_q24(const float* A, const uint16_t* Wh, float wscale, const float* bias, void* img,
                         int32_t plane_rows, int32_t M, int32_t N, int32_t K, int32_t norm, void* stream) {
  if (!Wh || !img || plane_rows < M) return fail(ND_ERR_ARG, "gemm_split_q24: null Wh / image, or plane_rows < M");
  nd::GemmArgs g{.A = A, .lda = K, .ldw = K, .bias = bias, .ldc = N, .norm = norm != 0, .M = M, .N = N, .K = K,
                 .Wh = Wh, .wscale = wscale, .q24 = static_cast<uint8_t*>(img),
                 .q24_plane = (size_t)plane_rows * CTXQ_ROW};
  return status("gemm_split_q24", nd::launch_gemm(g, (hipStream_t)stream));
}

static int ensure_attributes() {
  static hipError_t e = nd::init_kernel_attributes();
  return e == hipSuccess ? ND_OK : fail(ND_ERR_HIP, "hipFuncSetAttribute failed");
}

int nd_op_dec_ffn(const float* y, const uint16_t* w1h, float w1s, const float* b1, const uint16_t* w2h, float w2s,
                  const float* b2, float* x, float* xpart, int32_t M, int32_t F, int32_t nsplit, float* slab,
                  int32_t* tickets, const int32_t* skip, int32_t skip_rpc, int32_t* overflow, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  return status("dec_ffn", nd::launch_dec_ffn({.y = y, .w1h = w1h, .w1s = w1s, .b1 = b1, .w2h = w2h, .w2s = w2s,
                                               .b2 = b2, .x = x, .xpart = xpart, .M = M, .F = F, .ovf = overflow},
                                              {.nsplit = nsplit, .slab = slab, .tickets = tickets, .skip = skip,
                                               .skip_rpc = skip_rpc}, (hipStream_t)stream));
}

int64_t nd_op_dec_ffn_slab_floats(int32_t M, int32_t nsplit) {
  return M > 0 && nsplit > 0 ? (int64_t)nd::dec_ffn_slab_floats(M, nsplit) : 0;
}

int nd_op_gemm_p16(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M,
                   int32_t N, int32_t K, const float* part_in, int32_t part_n_in, float* part_out, int32_t relu,
                   int32_t* part_n_out, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  return status_p16("gemm_p16", {.A = A, .W = W, .bias = bias, .R = R, .C = C, .norm = part_in != nullptr, .M = M,
                                 .N = N, .K = K, .relu = relu != 0, .part_out = part_out, .part_in = part_in,
                                 .part_n_in = part_n_in}, part_n_out, stream);
}

int nd_op_pack_p16h(const float* W, int32_t N, int32_t K, uint16_t* out, float* wscale, void* stream) {
  return status("pack_p16h", nd::launch_pack_p16h(W, K, N, K, out, wscale, (hipStream_t)stream));
}

int nd_op_enc_ffn(const float* y, const uint16_t* w1h, float w1s, const float* b1, const uint16_t* w2h, float w2s,
                  const float* b2, float* x, float* xpart, int32_t M, int32_t F, int32_t* overflow, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  return status("enc_ffn", nd::launch_enc_ffn({.y = y, .w1h = w1h, .w1s = w1s, .b1 = b1, .w2h = w2h, .w2s = w2s,
                                               .b2 = b2, .x = x, .xpart = xpart, .M = M, .F = F, .ovf = overflow},
                                              {}, {}, (hipStream_t)stream));
}

int nd_op_enc_ffn_wo(const float* att, const float* x_in, const uint16_t* woh, float wos, const float* bo,
                     const uint16_t* w1h, float w1s, const float* b1, const uint16_t* w2h, float w2s, const float* b2,
                     float* x, float* xpart, const uint16_t* qkvh, float qkvs, const float* qkvb, float* qkv,
                     int32_t M, int32_t F, int32_t* overflow, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!att && M > 0) return status("enc_ffn_wo", hipErrorInvalidValue);  // this entry is the Wo fold: att is not optional
  return status("enc_ffn_wo",
                nd::launch_enc_ffn({.y = x_in, .w1h = w1h, .w1s = w1s, .b1 = b1, .w2h = w2h, .w2s = w2s, .b2 = b2,
                                    .x = x, .xpart = xpart, .M = M, .F = F, .ovf = overflow},
                                   {.att = att, .woh = woh, .wos = wos, .bo = bo},
                                   {.wh = qkvh, .ws = qkvs, .bias = qkvb, .out = qkv}, (hipStream_t)stream));
}

int nd_op_gemm_p16_split(const float* A, const uint16_t* Wh, float wscale, const float* bias, const float* R, float* C,
                         int32_t M, int32_t N, int32_t K, const float* part_in, int32_t part_n_in, float* part_out,
                         int32_t relu, int32_t* part_n_out, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!Wh) return fail(ND_ERR_ARG, "gemm_p16_split: null Wh");
  return status_p16("gemm_p16_split", {.A = A, .bias = bias, .R = R, .C = C, .norm = part_in != nullptr, .M = M,
                                       .N = N, .K = K, .relu = relu != 0, .part_out = part_out, .part_in = part_in,
                                       .part_n_in = part_n_in, .Wh = Wh, .wscale = wscale}, part_n_out, stream);
}

static int gemm_p16_splitk(const float* A, const uint16_t* Wh, const float* W, float wscale, const float* bias,
                           const float* R, float* C, int32_t M, int32_t N, int32_t K, float* part_out, float* slab,
                           int32_t* tickets, int32_t tiles, int32_t* part_n_out, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!A || (!Wh && !W) || !C || !slab || !tickets || tiles < 1)
    return fail(ND_ERR_ARG, "gemm_p16_splitk: bad arguments");
  if ((K != 1024 && K != 2048) || N % 32 || M <= 128 || ((M + 31) / 32) * (N / 32) > tiles)
    return fail(ND_ERR_ARG, "gemm_p16_splitk: needs K 1024 / 2048, N % 32 == 0, M > 128 and enough tiles");
  const long long before = nd::gemm_route_count(ND_ROUTE_P16_SPLITK, false);
  const int rc = status_p16("gemm_p16_splitk", {.A = A, .W = W, .bias = bias, .R = R, .C = C, .M = M, .N = N, .K = K,
                                                .part_out = part_out, .Wh = Wh, .wscale = wscale, .sk_slab = slab,
                                                .sk_cnt = tickets, .sk_tiles = tiles}, part_n_out, stream);
  if (rc != ND_OK) return rc;
  if (nd::gemm_route_count(ND_ROUTE_P16_SPLITK, false) == before) return fail(ND_ERR_ARG, "gemm_p16_splitk: not taken");
  return ND_OK;
}

int nd_op_gemm_p16_splitk(const float* A, const uint16_t* Wh, float wscale, const float* bias, const float* R,
                          float* C, int32_t M, int32_t N, int32_t K, float* part_out, float* slab, int32_t* tickets,
                          int32_t tiles, int32_t* part_n_out, void* stream) {
  if (!Wh) return fail(ND_ERR_ARG, "gemm_p16_splitk: null Wh");
  return gemm_p16_splitk(A, Wh, nullptr, wscale, bias, R, C, M, N, K, part_out, slab, tickets, tiles, part_n_out,
                         stream);
}

int nd_op_gemm_p16_splitk_f32(const float* A, const float* W, const float* bias, const float* R, float* C,
                              int32_t M, int32_t N, int32_t K, float* part_out, float* slab, int32_t* tickets,
                              int32_t tiles, int32_t* part_n_out, void* stream) {
  if (!W) return fail(ND_ERR_ARG, "gemm_p16_splitk_f32: null W");
  return gemm_p16_splitk(A, nullptr, W, 1.0f, bias, R, C, M, N, K, part_out, slab, tickets, tiles, part_n_out,
                         stream);
}

int nd_op_gemm_p16_split_rm(const float* A, const uint16_t* Wh, float wscale, const uint16_t* Wh_rm, float wscale_rm,
                            const float* bias, const float* R, float* C, int32_t M, int32_t N, int32_t K,
                            const float* part_in, int32_t part_n_in, float* part_out, int32_t relu,
                            int32_t* part_n_out, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!Wh || !Wh_rm) return fail(ND_ERR_ARG, "gemm_p16_split_rm: null weight image");
  return status_p16("gemm_p16_split_rm",
                    {.A = A, .bias = bias, .R = R, .C = C, .norm = part_in != nullptr, .M = M, .N = N, .K = K,
                     .relu = relu != 0, .part_out = part_out, .part_in = part_in, .part_n_in = part_n_in, .Wh = Wh,
                     .wscale = wscale, .Wh_rm = Wh_rm, .wscale_rm = wscale_rm}, part_n_out, stream);
}

int nd_op_pack_p16(const float* src, float* dst, int32_t M, int32_t N, void* stream) {
  return status("pack_p16", nd::launch_pack_p16(src, N, dst, M, N, (hipStream_t)stream));
}

int nd_op_fold_layernorm(const float* W, const float* bias, const float* ln_g, const float* ln_b, float* W_out,
                         float* b_out, int32_t N, int32_t K, void* stream) {
  return status("fold_layernorm", nd::launch_fold_layernorm(W, bias, ln_g, ln_b, W_out, b_out, N, K, (hipStream_t)stream));
}

int nd_op_enc_attention(const float* qkv, const float* signal, const int32_t* span, float* out, int32_t B, int32_t T,
                        void* stream) {
  return status("enc_attention", nd::launch_enc_attention({.qkv = qkv, .mask = {signal, span}, .out = out, .B = B,
                                                           .T = T}, (hipStream_t)stream));
}

int nd_op_enc_attention_ex(const float* qkv, const float* signal, const int32_t* span, float* out, int32_t B,
                           int32_t T, int32_t exact, int32_t* overflow, void* stream) {
  if (!qkv || !signal || !span || !out || B < 1) return fail(ND_ERR_ARG, "enc_attention_ex: bad arguments");
  return status("enc_attention_ex", nd::launch_enc_attention({.qkv = qkv, .mask = {signal, span}, .out = out, .B = B,
                                                              .T = T, .exact = exact != 0, .ovf = overflow},
                                                             (hipStream_t)stream));
}

int nd_op_enc_layer0(const float* signal, const int32_t* span, const float* w_in, const float* b_in,
                     const float* nwqkv, const float* nbqkv, float* out, int32_t B, int32_t T, float* ac_out,
                     double* scal_out, float* coef_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!signal || !span || !w_in || !b_in || !nwqkv || !nbqkv || !out || B < 1 || T < 1 || T > 512)
    return status("enc_layer0", hipErrorInvalidValue);  // launch_enc_attention_rank2's limit, checked before the prep launch
  // the engine's own preparation (nd_finalize's) into a workspace of this call
  const size_t n_ac = 6 * ND_D, n_coef = ND_H * 6;
  char* ws = nullptr;
  hipError_t e = hipMalloc((void**)&ws, 4 * sizeof(double) + (n_ac + n_coef) * sizeof(float));
  if (e != hipSuccess) return status("enc_layer0", e, ND_ERR_HIP);
  double* scal = reinterpret_cast<double*>(ws);
  float *ac = reinterpret_cast<float*>(scal + 4), *coef = ac + n_ac;
  nd::EmbedQkv eq;
  e = nd::prepare_embed_qkv(w_in, b_in, nwqkv, nbqkv, ac, scal, coef, &eq, s);
  if (e == hipSuccess) e = nd::launch_enc_attention_rank2({.signal = signal, .span = span, .eq = eq, .coef = coef,
                                                           .out = out}, B, T, s);
  if (e == hipSuccess && ac_out) e = hipMemcpyAsync(ac_out, ac, n_ac * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && scal_out) e = hipMemcpyAsync(scal_out, scal, 4 * sizeof(double), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && coef_out) e = hipMemcpyAsync(coef_out, coef, n_coef * sizeof(float), hipMemcpyDeviceToDevice, s);
  const hipError_t es = hipStreamSynchronize(s);  // the workspace is read until here
  (void)hipFree(ws);
  return status("enc_layer0", e != hipSuccess ? e : es, ND_ERR_HIP);
}

int nd_op_dec_self_attention(const float* qkv, float* cache, const int32_t* anc, int32_t anc_ld, int32_t step,
                             int32_t max_steps, float* out, int32_t R, void* stream) {
  return status("dec_self_attention",
                nd::launch_dec_self_attention({.qkv = qkv, .cache = cache, .anc = anc, .anc_ld = anc_ld, .step = step,
                                               .max_steps = max_steps, .out = out, .R = R}, (hipStream_t)stream));
}

int nd_op_dec_self_attention_beam(const float* qkv, float* cache, const int32_t* anc, int32_t anc_ld, int32_t step,
                                  int32_t max_steps, float* out, int32_t R, int32_t rpc, const int32_t* done,
                                  void* stream) {
  if (!qkv || !cache || !anc || !out || rpc < 2 || rpc > 8 || R % rpc)
    return fail(ND_ERR_ARG, "dec_self_attention_beam: bad arguments");
  return status("dec_self_attention_beam",
                nd::launch_dec_self_attention({.qkv = qkv, .cache = cache, .anc = anc, .anc_ld = anc_ld, .step = step,
                                               .max_steps = max_steps, .out = out, .R = R,
                                               .rows = {.C = R / rpc, .rpc = rpc, .done = done}}, (hipStream_t)stream));
}

int nd_op_dec_self_attention_q24(const float* qkv, void* cache, const int32_t* anc, int32_t anc_ld, int32_t step,
                                 int32_t max_steps, float* out, int32_t R, int32_t rpc, const int32_t* done,
                                 void* stream) {
  if (!qkv || !cache || !out || rpc < 1 || rpc > 8 || R % rpc || (rpc > 1 && !anc))
    return fail(ND_ERR_ARG, "dec_self_attention_q24: bad arguments");
  return status("dec_self_attention_q24",
                nd::launch_dec_self_attention({.qkv = qkv, .cache = static_cast<float*>(cache), .anc = anc,
                                               .anc_ld = anc_ld, .step = step, .max_steps = max_steps, .out = out,
                                               .R = R, .rows = {.C = R / rpc, .rpc = rpc, .done = done}, .q24 = true},
                                              (hipStream_t)stream));
}

int nd_op_dec_self_attention_table(const float* table, int32_t table_steps, int32_t V, const int32_t* tok,
                                   int32_t tok0, const int32_t* hist, int32_t hist_ld, float* cache, int32_t step,
                                   int32_t max_steps, float* out, int32_t R, void* stream) {
  if (!table || !tok || !hist || !out || R < 1 || V < 1 || step < 0 || step >= table_steps)
    return fail(ND_ERR_ARG, "dec_self_attention_table: bad arguments");
  const nd::QkvRows qr{.tok = tok, .V = V, .tok0 = tok0, .rm = 1, .hist = hist, .hist_ld = hist_ld};
  return status("dec_self_attention_table",
                nd::launch_dec_self_attention({.qkv = table, .cache = cache, .step = step, .max_steps = max_steps,
                                               .out = out, .R = R, .rows = {.C = R}, .qr = qr}, (hipStream_t)stream));
}

int nd_op_dec_mem_attention(const float* qp, const float* mem, const float* signal, const int32_t* span, float pad_val,
                            float* out, int32_t C, int32_t rpc, int32_t T, int32_t ldT, int32_t grid, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  return status("dec_mem_attention",
                nd::launch_dec_mem_attention({.qp = qp, .mem = mem, .mask = {signal, span, pad_val}, .out = out, .C = C,
                                              .rpc = rpc, .T = T, .ldT = ldT, .grid = grid}, (hipStream_t)stream));
}

static int lstm_layer(const float* xp, const float* signal, const float* wih0, const float* bsum, const float* whh,
                      const int32_t* len, int32_t B, int32_t T, float* out, const float* bn_scale,
                      const float* bn_shift, int32_t layer0, bool exact, void* stream) {
  if (B < 1 || T < 1 || !whh || !len || !out || (layer0 ? (!signal || !wih0 || !bsum) : !xp))
    return fail(ND_ERR_ARG, "lstm_layer: bad arguments");
  if ((bn_scale == nullptr) != (bn_shift == nullptr))
    return fail(ND_ERR_ARG, "lstm_layer: bn_scale and bn_shift must both be set or both be null");
  return status("lstm_layer",
                nd::launch_lstm_layer({.xp = xp, .signal = signal, .wih0 = wih0, .bsum = bsum, .whh = whh, .len = len,
                                       .B = B, .T = T, .out = out, .bn_scale = bn_scale, .bn_shift = bn_shift,
                                       .layer0 = layer0 != 0, .exact = exact}, (hipStream_t)stream));
}

int nd_op_lstm_layer(const float* xp, const float* signal, const float* wih0, const float* bsum, const float* whh,
                     const int32_t* len, int32_t B, int32_t T, float* out, const float* bn_scale,
                     const float* bn_shift, int32_t layer0, void* stream) {
  return lstm_layer(xp, signal, wih0, bsum, whh, len, B, T, out, bn_scale, bn_shift, layer0, false, stream);
}

int nd_op_lstm_layer_f32(const float* xp, const float* signal, const float* wih0, const float* bsum, const float* whh,
                         const int32_t* len, int32_t B, int32_t T, float* out, const float* bn_scale,
                         const float* bn_shift, int32_t layer0, void* stream) {
  return lstm_layer(xp, signal, wih0, bsum, whh, len, B, T, out, bn_scale, bn_shift, layer0, true, stream);
}

int nd_normalize_reads(const double* d_raw, const int64_t* d_offsets, int32_t R, int32_t method, float* d_out,
                       void* stream) {
  return status("normalize_reads",
                nd::launch_read_normalize(d_raw, (const long long*)d_offsets, R, method, d_out, (hipStream_t)stream));
}

int nd_window_reads(const float* d_sig, const int64_t* d_offsets, const int32_t* d_read, const int32_t* d_start,
                    const int32_t* d_len, int32_t C, int32_t T, float* d_signal, void* stream) {
  return status("window_reads", nd::launch_read_window(d_sig, (const long long*)d_offsets, d_read, d_start, d_len, C, T,
                                                       d_signal, (hipStream_t)stream));
}

// The four forms of read assembly: ``name`` the entry without its nd_ prefix, q / m / p the form (which optional
// pairs of ``a`` the entry has); a.total is set here, from total_bases once it is known to fit.
static int assemble_entry(const char* name, bool q, bool m, bool p, nd::AsmArgs a, int64_t total_bases,
                          int64_t work_bytes, void* stream) {
  const std::string n(name);
  if (a.R < 0 || a.C < 0 || total_bases < 0 || total_bases >= (int64_t)1 << 31)
    return fail(ND_ERR_ARG, n + ": R, C and total_bases must be >= 0 and total_bases < 2^31");
  const int64_t need = (int64_t)nd::assemble_work_bytes(a.C, total_bases, q, m, p);
  if (work_bytes < need)
    return fail(ND_ERR_ARG, n + ": work_bytes " + std::to_string(work_bytes) + " below the " + std::to_string(need) +
                                " nd_" + n + "_work_bytes asks for");
  if (!a.chunk_off || !a.read_off || (a.R > 0 && (!a.seq_len || !a.status)) || (need > 0 && !a.work) ||
      (total_bases > 0 && (!a.bases || !a.seq || (q && (!a.qw || !a.qual)) || (m && (!a.mw || !a.ml)) ||
                           (p && (!a.bp || !a.rpos)))))
    return fail(ND_ERR_ARG, n + ": null buffer");
  if (a.R == 0) return ND_OK;
  a.total = (int)total_bases;
  if (total_bases == 0) {  // no base to weigh or to place: the plain form's paths (no chunks, or only empty ones)
    a.qw = a.mw = nullptr;
    a.qual = a.ml = nullptr;
    a.bp = nullptr;
    a.rpos = nullptr;
  }
  return status(name, nd::launch_assemble_reads(a, (hipStream_t)stream), ND_ERR_HIP);
}

int64_t nd_assemble_reads_work_bytes(int32_t C, int64_t total_bases) {
  return C >= 0 && total_bases >= 0 ? (int64_t)nd::assemble_work_bytes(C, total_bases, false, false, false) : -1;
}

int nd_assemble_reads(const uint8_t* d_bases, const int32_t* d_chunk_off, const int32_t* d_read_off, int32_t R,
                      int32_t C, int64_t total_bases, uint8_t* d_seq, int32_t* d_seq_len, int32_t* d_status,
                      void* d_work, int64_t work_bytes, void* stream) {
  nd::AsmArgs a{.bases = d_bases, .chunk_off = d_chunk_off, .read_off = d_read_off, .R = R, .C = C, .seq = d_seq,
                .seq_len = d_seq_len, .status = d_status, .work = d_work};
  return assemble_entry("assemble_reads", false, false, false, a, total_bases, work_bytes, stream);
}

int64_t nd_assemble_reads_q_work_bytes(int32_t C, int64_t total_bases) {
  return C >= 0 && total_bases >= 0 ? (int64_t)nd::assemble_work_bytes(C, total_bases, true, false, false) : -1;
}

int nd_assemble_reads_q(const uint8_t* d_bases, const uint16_t* d_qw, const int32_t* d_chunk_off,
                        const int32_t* d_read_off, int32_t R, int32_t C, int64_t total_bases, uint8_t* d_seq,
                        uint8_t* d_qual, int32_t* d_seq_len, int32_t* d_status, void* d_work, int64_t work_bytes,
                        void* stream) {
  nd::AsmArgs a{.bases = d_bases, .chunk_off = d_chunk_off, .read_off = d_read_off, .R = R, .C = C, .seq = d_seq,
                .seq_len = d_seq_len, .status = d_status, .work = d_work, .qw = d_qw, .qual = d_qual};
  return assemble_entry("assemble_reads_q", true, false, false, a, total_bases, work_bytes, stream);
}

int nd_token_weights(const int32_t* d_tokens, const float* d_logp, const float* d_tok_logp, int32_t B, int32_t S,
                     int32_t V, uint16_t* d_w, void* stream) {
  if (B < 0 || S < 0 || V < 1 || (int64_t)B * S >= (int64_t)1 << 31)
    return fail(ND_ERR_ARG, "token_weights: B and S must be >= 0, V >= 1 and B * S < 2^31");
  if ((d_logp != nullptr) == (d_tok_logp != nullptr))
    return fail(ND_ERR_ARG, "token_weights: exactly one of d_logp and d_tok_logp must be given");
  if ((int64_t)B * S > 0 && (!d_tokens || !d_w)) return fail(ND_ERR_ARG, "token_weights: null buffer");
  return status("token_weights", nd::launch_token_weights(d_tokens, d_logp, d_tok_logp, B * S, V, d_w,
                                                          (hipStream_t)stream), ND_ERR_HIP);
}

int nd_token_mod_weights(const int32_t* d_tokens, const float* d_logp, int32_t B, int32_t S, int32_t V,
                         int32_t canon_id, int32_t mod_id, uint16_t* d_mw, void* stream) {
  if (B < 0 || S < 0 || V < 1 || (int64_t)B * S >= (int64_t)1 << 31)
    return fail(ND_ERR_ARG, "token_mod_weights: B and S must be >= 0, V >= 1 and B * S < 2^31");
  if (canon_id < 0 || canon_id >= V || mod_id < 0 || mod_id >= V || canon_id == mod_id)
    return fail(ND_ERR_ARG, "token_mod_weights: canon_id and mod_id must be two different ids in [0, V)");
  if ((int64_t)B * S > 0 && (!d_tokens || !d_logp || !d_mw)) return fail(ND_ERR_ARG, "token_mod_weights: null buffer");
  return status("token_mod_weights", nd::launch_token_mod_weights(d_tokens, d_logp, B * S, V, canon_id, mod_id, d_mw,
                                                                  (hipStream_t)stream), ND_ERR_HIP);
}

int64_t nd_assemble_reads_m_work_bytes(int32_t C, int64_t total_bases) {
  return C >= 0 && total_bases >= 0 ? (int64_t)nd::assemble_work_bytes(C, total_bases, true, true, false) : -1;
}

int nd_assemble_reads_m(const uint8_t* d_bases, const uint16_t* d_qw, const uint16_t* d_mw,
                        const int32_t* d_chunk_off, const int32_t* d_read_off, int32_t R, int32_t C,
                        int64_t total_bases, uint8_t* d_seq, uint8_t* d_qual, uint8_t* d_ml, int32_t* d_seq_len,
                        int32_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
  nd::AsmArgs a{.bases = d_bases, .chunk_off = d_chunk_off, .read_off = d_read_off, .R = R, .C = C, .seq = d_seq,
                .seq_len = d_seq_len, .status = d_status, .work = d_work, .qw = d_qw, .qual = d_qual,
                .mw = d_mw, .ml = d_ml};
  return assemble_entry("assemble_reads_m", true, true, false, a, total_bases, work_bytes, stream);
}

int nd_token_positions(const float* d_attn, int64_t ld_chunk, const int32_t* d_span, int32_t B, int32_t S, int32_t T,
                       int32_t* d_pos, void* stream) {
  if (B < 0 || S < 0 || T < 1 || T > TOKEN_POS_MAX_T || (int64_t)B * S >= (int64_t)1 << 31)
    return fail(ND_ERR_ARG, "token_positions: B and S must be >= 0, T in [1, 2^19] and B * S < 2^31");
  if (ld_chunk < (int64_t)S * T) return fail(ND_ERR_ARG, "token_positions: ld_chunk below S * T");
  if ((B > 0 && !d_span) || ((int64_t)B * S > 0 && (!d_attn || !d_pos)))
    return fail(ND_ERR_ARG, "token_positions: null buffer");
  return status("token_positions", nd::launch_token_positions(d_attn, ld_chunk, d_span, B, S, T, d_pos,
                                                              (hipStream_t)stream), ND_ERR_HIP);
}

int nd_cand_posterior(const float* d_score, const int32_t* d_cand_len, int32_t B, int32_t K, float* d_score_out,
                      float* d_post, int32_t* d_best, void* stream) {
  if (B < 0 || K < 1 || (int64_t)B * K >= (int64_t)1 << 31)
    return fail(ND_ERR_ARG, "cand_posterior: B must be >= 0, K >= 1 and B * K < 2^31");
  if (B == 0) return ND_OK;
  if (!d_score || !d_cand_len || !d_score_out) return fail(ND_ERR_ARG, "cand_posterior: null buffer");
  return status("cand_posterior", nd::launch_cand_posterior(d_score, d_cand_len, B, K, d_score_out, d_post, d_best,
                                                            (hipStream_t)stream), ND_ERR_HIP);
}

int64_t nd_assemble_reads_p_work_bytes(int32_t C, int64_t total_bases) {
  return C >= 0 && total_bases >= 0 ? (int64_t)nd::assemble_work_bytes(C, total_bases, false, false, true) : -1;
}

int nd_assemble_reads_p(const uint8_t* d_bases, const uint32_t* d_bp, const int32_t* d_chunk_off,
                        const int32_t* d_read_off, int32_t R, int32_t C, int64_t total_bases, uint8_t* d_seq,
                        uint32_t* d_rpos, int32_t* d_seq_len, int32_t* d_status, void* d_work, int64_t work_bytes,
                        void* stream) {
  nd::AsmArgs a{.bases = d_bases, .chunk_off = d_chunk_off, .read_off = d_read_off, .R = R, .C = C, .seq = d_seq,
                .seq_len = d_seq_len, .status = d_status, .work = d_work, .bp = d_bp, .rpos = d_rpos};
  return assemble_entry("assemble_reads_p", false, false, true, a, total_bases, work_bytes, stream);
}

int64_t nd_align_seqs_work_bytes(int32_t P, int64_t cells) {
  return P >= 0 && cells >= 0 && cells <= ALIGN_MAX_CELLS ? (int64_t)nd::align_work_bytes(P, cells) : -1;
}

// The argument checks of nd_align_seqs, nd_align_fit and nd_align_fit_pos, in the order every one of them tests:
// the sizes (``ref_len`` null for nd_align_seqs, which has none), P == 0 (ND_OK, nothing to launch), the work
// area's size, the required buffers (``d_work`` among them) and the work area's alignment.  ``launch`` is set
// when the entry is to go on.
static int align_check(const char* entry, const int32_t* ref_len, int32_t P, int64_t cells, int64_t work_bytes,
                       const void* d_work, std::initializer_list<const void*> required, bool& launch) {
  const std::string name(entry);
  launch = false;
  if (P < 0 || cells < 0 || cells > ALIGN_MAX_CELLS || (ref_len && *ref_len < 0))
    return fail(ND_ERR_ARG, name + (ref_len ? ": P, cells and ref_len" : ": P and cells") +
                                " must be >= 0 and cells <= 2^60");
  if (P == 0) return ND_OK;
  const int64_t need = (int64_t)nd::align_work_bytes(P, cells);
  if (work_bytes < need)
    return fail(ND_ERR_ARG, name + ": work_bytes " + std::to_string(work_bytes) + " below the " +
                                std::to_string(need) + " nd_" + name + "_work_bytes asks for");
  for (const void* b : required)
    if (!b) return fail(ND_ERR_ARG, name + ": null buffer");
  if (reinterpret_cast<uintptr_t>(d_work) & 7) return fail(ND_ERR_ARG, name + ": d_work must be 8-byte aligned");
  launch = true;
  return ND_OK;
}

int nd_align_seqs(const uint8_t* d_call, const int32_t* d_call_off, const uint8_t* d_truth,
                  const int32_t* d_truth_off, int32_t P, int64_t cells, int32_t* d_counts, uint8_t* d_ops,
                  int32_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
  bool launch;
  const int rc = align_check("align_seqs", nullptr, P, cells, work_bytes, d_work,
                             {d_call, d_call_off, d_truth, d_truth_off, d_counts, d_status, d_work}, launch);
  if (!launch) return rc;
  return status("align_seqs", nd::launch_align_seqs(d_call, d_call_off, d_truth, d_truth_off, P, cells, d_counts,
                                                    d_ops, d_status, d_work, (hipStream_t)stream), ND_ERR_HIP);
}

int nd_locate_segs(const uint8_t* d_call, const int32_t* d_call_off, int32_t P, const uint32_t* d_idx_code,
                   const uint32_t* d_idx_pos, int32_t idx_len, const int32_t* d_rec_off, int32_t R, int32_t* d_hit,
                   int32_t* d_status, uint8_t* d_call_or, void* stream) {
  if (P < 0 || idx_len < 0 || R < 0) return fail(ND_ERR_ARG, "locate_segs: P, idx_len and R must be >= 0");
  if (P == 0) return ND_OK;
  if (!d_call || !d_call_off || !d_rec_off || !d_hit || !d_status || !d_call_or ||
      (idx_len > 0 && (!d_idx_code || !d_idx_pos)))
    return fail(ND_ERR_ARG, "locate_segs: null buffer");
  if (d_call == d_call_or) return fail(ND_ERR_ARG, "locate_segs: d_call_or must not be d_call");
  return status("locate_segs", nd::launch_locate_segs(d_call, d_call_off, P, d_idx_code, d_idx_pos, idx_len, d_rec_off,
                                                      R, d_hit, d_status, d_call_or, (hipStream_t)stream), ND_ERR_HIP);
}

int64_t nd_align_fit_work_bytes(int32_t P, int64_t cells) { return nd_align_seqs_work_bytes(P, cells); }

int nd_align_fit(const uint8_t* d_call_or, const int32_t* d_call_off, const uint8_t* d_ref, int32_t ref_len,
                 const int32_t* d_hit, int32_t P, int64_t cells, int32_t* d_counts, int32_t* d_span, uint8_t* d_ops,
                 int32_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
  bool launch;
  const int rc = align_check("align_fit", &ref_len, P, cells, work_bytes, d_work,
                             {d_call_or, d_call_off, d_ref, d_hit, d_counts, d_span, d_status, d_work}, launch);
  if (!launch) return rc;
  return status("align_fit", nd::launch_align_fit(d_call_or, d_call_off, d_ref, ref_len, d_hit, P, cells, d_counts,
                                                  d_span, d_ops, d_status, nullptr, d_work, (hipStream_t)stream),
                ND_ERR_HIP);
}

int64_t nd_align_fit_pos_work_bytes(int32_t P, int64_t cells) { return nd_align_seqs_work_bytes(P, cells); }

int nd_align_fit_pos(const uint8_t* d_call_or, const int32_t* d_call_off, const uint8_t* d_ref, int32_t ref_len,
                     const int32_t* d_hit, int32_t P, int64_t cells, int32_t* d_counts, int32_t* d_span,
                     uint8_t* d_ops, int32_t* d_rpos, int32_t* d_status, void* d_work, int64_t work_bytes,
                     void* stream) {
  bool launch;  // d_rpos is required here: the launcher takes a null one for the form without positions
  const int rc = align_check("align_fit_pos", &ref_len, P, cells, work_bytes, d_work,
                             {d_call_or, d_call_off, d_ref, d_hit, d_counts, d_span, d_rpos, d_status, d_work}, launch);
  if (!launch) return rc;
  return status("align_fit_pos", nd::launch_align_fit(d_call_or, d_call_off, d_ref, ref_len, d_hit, P, cells,
                                                      d_counts, d_span, d_ops, d_status, d_rpos, d_work,
                                                      (hipStream_t)stream), ND_ERR_HIP);
}

int nd_pileup_add(const uint8_t* d_call_or, const int32_t* d_call_off, const uint8_t* d_ops, const int32_t* d_rpos,
                  const int32_t* d_status, int32_t P, uint32_t* d_pile, int32_t ref_len, void* stream) {
  if (P < 0 || ref_len < 0) return fail(ND_ERR_ARG, "pileup_add: P and ref_len must be >= 0");
  if (P == 0 || ref_len == 0) return ND_OK;
  if (!d_call_or || !d_call_off || !d_ops || !d_rpos || !d_status || !d_pile)
    return fail(ND_ERR_ARG, "pileup_add: null buffer");
  return status("pileup_add", nd::launch_pileup_add(d_call_or, d_call_off, d_ops, d_rpos, d_status, P, d_pile,
                                                    ref_len, (hipStream_t)stream), ND_ERR_HIP);
}

int nd_pileup_call(const uint32_t* d_pile, const uint8_t* d_ref, int32_t ref_len, const int32_t* d_rec_off, int32_t R,
                   int32_t min_cov, uint8_t* d_cons, uint8_t* d_ins, int32_t* d_cov, int64_t* d_rec, void* stream) {
  if (ref_len < 0 || R < 0 || min_cov < 1)
    return fail(ND_ERR_ARG, "pileup_call: ref_len and R must be >= 0 and min_cov >= 1");
  if (R == 0 || ref_len == 0) return ND_OK;
  if (!d_pile || !d_ref || !d_rec_off || !d_cons || !d_ins || !d_cov || !d_rec)
    return fail(ND_ERR_ARG, "pileup_call: null buffer");
  return status("pileup_call", nd::launch_pileup_call(d_pile, d_ref, ref_len, d_rec_off, R, min_cov, d_cons, d_ins,
                                                      d_cov, reinterpret_cast<long long*>(d_rec),
                                                      (hipStream_t)stream), ND_ERR_HIP);
}

int nd_phred_ratios(double* out, int32_t n) {
  if (!out || n < 0 || n > PHRED_LEVELS) return fail(ND_ERR_ARG, "phred_ratios: out null, or n outside [0, 41]");
  for (int k = 0; k < n; ++k) out[k] = nd::phred_ratios()[k];
  return ND_OK;
}

int nd_op_memory_pack(const float* x, const float* ln_g, const float* ln_b, float* out, int32_t B, int32_t T,
                      int32_t ldT, void* stream) {
  return status("memory_pack", nd::launch_memory_pack(x, ln_g, ln_b, out, B, T, ldT, (hipStream_t)stream));
}

int nd_op_bank_pack_d8(const float* x, const float* ln_g, const float* ln_b, void* bank, float* kscale,
                       int32_t* kemax, const int32_t* span, int32_t B, int32_t T, int32_t* ovf, void* stream) {
  if (!x || !bank || !kscale || !kemax || (ln_g == nullptr) != (ln_b == nullptr))
    return fail(ND_ERR_ARG, "bank_pack_d8: bad arguments");
  return status("bank_pack_d8",
                nd::launch_bank_pack_d8({.x = x, .ln_g = ln_g, .ln_b = ln_b, .bank = bank, .kscale = kscale,
                                         .kemax = kemax, .span = span, .B = B, .T = T, .ovf = ovf}, (hipStream_t)stream));
}

int nd_op_dec_bank_d8(const float* qp, const void* bank, const float* kscale, const int32_t* kemax,
                      const float* signal, const int32_t* span, float pad_val, float* out, int32_t C, int32_t T,
                      int32_t* ovf, int32_t grid, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!qp || !bank || !kscale || !kemax || !signal || !span || !out || grid < 0)
    return fail(ND_ERR_ARG, "dec_bank_d8: bad arguments");
  return status("dec_bank_d8",
                nd::launch_dec_bank_d8({.qp = qp, .bank = bank, .kscale = kscale, .kemax = kemax,
                                        .mask = {signal, span, pad_val}, .out = out, .C = C, .T = T, .ovf = ovf,
                                        .grid = grid}, (hipStream_t)stream));
}

int nd_op_dec_ctx_attention(const float* q, const float* kv, int32_t ld, int32_t koff, const float* signal,
                            const int32_t* span, float pad_val, float* out, int32_t C, int32_t rpc, int32_t T,
                            void* stream) {
  if (int rc = ensure_attributes()) return rc;
  return status("dec_ctx_attention",
                nd::launch_dec_ctx_attention({.q = q, .kv = kv, .ld = ld, .koff = koff, .T = T, .out = out,
                                              .mask = {signal, span, pad_val}, .rows = {.C = C, .rpc = rpc}},
                                             (hipStream_t)stream));
}

int nd_op_tf_attention(const float* q, int32_t ldq, const float* kv, int32_t ldkv, int32_t koff, int32_t voff,
                       const float* signal, const int32_t* span, float pad_val, float* out, int32_t B, int32_t Lq,
                       int32_t Lk, int32_t causal, void* stream) {
  return status("tf_attention",
                nd::launch_tf_attention({.q = q, .ldq = ldq, .kv = kv, .ldkv = ldkv, .koff = koff, .voff = voff,
                                         .mask = {signal, span, pad_val}, .out = out, .B = B, .Lq = Lq, .Lk = Lk,
                                         .causal = causal != 0}, (hipStream_t)stream));
}

int nd_op_tf_attention_tap(const float* q, int32_t ldq, const float* kv, int32_t ldkv, int32_t koff, int32_t voff,
                           const float* signal, const int32_t* span, float pad_val, float* out, int32_t B, int32_t Lq,
                           int32_t Lk, int32_t causal, float* tap, int32_t ld_tap, void* stream) {
  if (causal != 0) return fail(ND_ERR_ARG, "tf_attention_tap: the tap is the context attention's (causal must be 0)");
  if (!tap) return fail(ND_ERR_ARG, "tf_attention_tap: null tap");
  if (ld_tap < Lk) return fail(ND_ERR_ARG, "tf_attention_tap: ld_tap below Lk");
  return status("tf_attention_tap",
                nd::launch_tf_attention({.q = q, .ldq = ldq, .kv = kv, .ldkv = ldkv, .koff = koff, .voff = voff,
                                         .mask = {signal, span, pad_val}, .out = out, .B = B, .Lq = Lq, .Lk = Lk,
                                         .causal = false, .tap = tap, .ld_tap = ld_tap}, (hipStream_t)stream));
}

int nd_op_ctx_pack_q24(const float* kv, int32_t ld, int32_t layers, void* out, const int32_t* span, int32_t B,
                       int32_t T, void* stream) {
  if (!kv || !out || !span) return fail(ND_ERR_ARG, "ctx_pack_q24: bad arguments");
  return status("ctx_pack_q24",
                nd::launch_ctx_pack_q24(kv, ld, layers, static_cast<uint8_t*>(out), span, B, T, (hipStream_t)stream));
}

int nd_op_dec_ctx_attention_list(const float* q, const void* kv, int32_t ld, int32_t koff, int32_t q24,
                                 const float* signal, const int32_t* span, float pad_val, float* out, int32_t C,
                                 int32_t rpc, int32_t T, const int32_t* clist, int32_t ccap, int32_t nsplit,
                                 float* part, const int32_t* done, void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!q || !kv || !signal || !span || !out || !clist || (nsplit > 1 && !part))
    return fail(ND_ERR_ARG, "dec_ctx_attention_list: bad arguments");
  return status("dec_ctx_attention_list", nd::launch_dec_ctx_attention(
      {.q = q, .kv = kv, .ld = ld, .koff = koff, .q24 = q24 != 0, .T = T, .out = out, .mask = {signal, span, pad_val},
       .rows = {.C = C, .rpc = rpc, .done = done, .clist = clist, .ccap = ccap}, .nsplit = nsplit, .part = part},
      (hipStream_t)stream));
}

int nd_op_alive_list(const int32_t* done, int32_t C, int32_t* list, int32_t cap, int32_t* ovf, void* stream) {
  if (!done || !list) return fail(ND_ERR_ARG, "alive_list: bad arguments");
  return status("alive_list", nd::launch_alive_list(done, C, list, cap, ovf, (hipStream_t)stream));
}

int nd_op_dec_ctx_attention_q24(const float* q, const void* kvq, int32_t layers, int32_t layer, const float* signal,
                                const int32_t* span, float pad_val, float* out, int32_t C, int32_t rpc, int32_t T,
                                void* stream) {
  if (int rc = ensure_attributes()) return rc;
  if (!q || !kvq || !signal || !span || !out || layer < 0 || layer >= layers)
    return fail(ND_ERR_ARG, "dec_ctx_attention_q24: bad arguments");
  const uint8_t* plane = static_cast<const uint8_t*>(kvq) + (size_t)layer * C * T * CTXQ_ROW;
  return status("dec_ctx_attention_q24",
                nd::launch_dec_ctx_attention({.q = q, .kv = plane, .ld = CTXQ_ROW, .koff = 0, .q24 = true, .T = T,
                                              .out = out, .mask = {signal, span, pad_val},
                                              .rows = {.C = C, .rpc = rpc}}, (hipStream_t)stream));
}

// ---- output head and search (search.hip, head.hpp), one launch per call ----
static nd::BeamState beam_state(const nd_beam_state& a) {
  nd::BeamState st{};
  st.cum = a.cum;
  for (int i = 0; i < 2; ++i) {
    st.seq[i] = a.seq[i];
    st.anc[i] = a.anc[i];
    st.cov[i] = a.cov[i];
    st.blk[i] = a.blk[i];
  }
  st.tok = a.tok;
  st.done = a.done;
  st.top_fin = a.top_fin;
  st.n_hyp = a.n_hyp;
  st.hyp_score = a.hyp_score;
  st.hyp_len = a.hyp_len;
  st.hyp_tok = a.hyp_tok;
  st.n_alive = a.n_alive;
  st.steps_done = a.steps_done;
  st.group = a.group;
  st.grp_left = a.grp_left;
  st.grp_done = a.grp_done;
  st.steps_run = a.steps_run;
  st.hyp_anc = a.hyp_anc;
  st.pen = a.pen;
  st.prev_pen = a.prev_pen;
  st.attn = a.attn;
  st.cut = a.cut;
  st.T = a.T;
  return st;
}
// the members every beam kernel touches
static bool beam_state_ok(const nd_beam_state* a) {
  return a && a->cum && a->seq[0] && a->seq[1] && a->anc[0] && a->anc[1] && a->tok && a->done && a->top_fin &&
         a->n_hyp && a->hyp_score && a->hyp_len && a->hyp_tok && a->hyp_anc && a->n_alive && a->steps_done &&
         a->steps_run;
}
static bool classic_state_ok(const nd_beam_state* a) {
  return beam_state_ok(a) && a->group && a->grp_left && a->grp_done;
}
static nd::ClassicOpts classic_opts(const nd_classic_opts& op) {
  return {op.length_penalty, op.alpha, op.beta, op.coverage_penalty, op.stepwise_penalty, op.block_ngram_repeat,
          op.ignore_mask};
}
static bool classic_opts_ok(const nd_classic_opts* op) {
  return op && op->length_penalty >= 0 && op->length_penalty <= 2 && op->coverage_penalty >= 0 &&
         op->coverage_penalty <= 2;
}

int nd_op_greedy_head(const float* x, const float* ln_g, const float* ln_b, const float* gw, const float* gb, int32_t V,
                      int32_t S, int32_t step, int32_t min_len, int32_t eos, int32_t R, const float* emb,
                      const float* pe, float* ne_x, float* ne_part, int32_t* ne_tok, int32_t* tok,
                      int32_t* out_tokens, float* score, float* logp, float temp, int32_t topk,
                      const uint64_t* d_seed, void* stream) {
  if (!x || !ln_g || !ln_b || !gw || !gb || !emb || !ne_x || !ne_part || !tok || !out_tokens || !score || R < 1 ||
      S < 1 || step < 0 || step >= S || eos < 0 || (V >= 1 && eos >= V))
    return fail(ND_ERR_ARG, "greedy_head: bad arguments");
  const nd::GreedyHead h{.x = x, .ln_g = ln_g, .ln_b = ln_b, .gw = gw, .gb = gb, .V = V, .S = S, .min_len = min_len,
                         .eos = eos, .tok = tok, .out_tokens = out_tokens, .score = score, .logp_dump = logp,
                         .ne = {.emb = emb, .pe = pe, .x = ne_x, .part = ne_part, .tok = ne_tok},
                         .smp = {.temp = temp, .topk = topk,
                                 .seed = reinterpret_cast<const unsigned long long*>(d_seed)}};
  return status("greedy_head", nd::launch_dec_greedy_head(h, step, R, (hipStream_t)stream));
}

int nd_op_beam_init(const nd_beam_state* st, int32_t C, int32_t beam, int32_t bos, void* stream) {
  if (!beam_state_ok(st) || C < 1 || beam < 1 || beam > 8) return fail(ND_ERR_ARG, "beam_init: bad arguments");
  return status("beam_init", nd::launch_beam_init(beam_state(*st), C, beam, bos, (hipStream_t)stream));
}

int nd_op_beam_step(const float* x, const float* ln_g, const float* ln_b, const float* gw, const float* gb, int32_t V,
                    const float* emb, const float* pe, float* ne_x, float* ne_part, int32_t* ne_tok,
                    const nd_beam_state* st, int32_t C, int32_t beam, int32_t n_best, int32_t step, int32_t S,
                    int32_t min_len, int32_t eos, float alpha, const int32_t* clist, int32_t ccap, void* stream) {
  if (!x || !ln_g || !ln_b || !gw || !gb || !emb || !ne_x || !ne_part || !beam_state_ok(st) || C < 1 || S < 1 ||
      step < 0 || step >= S || eos < 0 || (V >= 1 && eos >= V))
    return fail(ND_ERR_ARG, "beam_step: bad arguments");
  const nd::BeamCall bc{.rows = {.C = C, .rpc = beam, .clist = clist, .ccap = ccap}, .n_best = n_best, .S = S,
                        .min_len = min_len, .eos = eos};
  return status("beam_step",
                nd::launch_beam_step({.emb = emb, .pe = pe, .x = ne_x, .part = ne_part, .tok = ne_tok},
                                     {.x = x, .ln_g = ln_g, .ln_b = ln_b, .gw = gw, .gb = gb, .V = V},
                                     beam_state(*st), bc, step, nd::fast_beam_lenpen(step, alpha),
                                     (hipStream_t)stream));
}

int nd_op_beam_finish(const nd_beam_state* st, int32_t C, int32_t n_best, int32_t S, int32_t* tokens, float* scores,
                      int32_t* lens, void* stream) {
  if (!beam_state_ok(st) || !tokens || !scores || !lens || C < 1 || n_best < 1 || S < 1)
    return fail(ND_ERR_ARG, "beam_finish: bad arguments");
  return status("beam_finish",
                nd::launch_beam_finish(beam_state(*st), C, n_best, S, tokens, scores, lens, (hipStream_t)stream));
}

int nd_op_beam_classic_init(const nd_beam_state* st, const int32_t* group, int32_t C, int32_t beam, int32_t bos,
                            void* stream) {
  if (!classic_state_ok(st) || !group || C < 1 || beam < 1 || beam > 8)
    return fail(ND_ERR_ARG, "beam_classic_init: bad arguments");
  return status("beam_classic_init",
                nd::launch_beam_classic_init(beam_state(*st), group, C, beam, bos, (hipStream_t)stream), ND_ERR_HIP);
}

int nd_op_beam_classic_step(const float* x, const float* ln_g, const float* ln_b, const float* gw, const float* gb,
                            int32_t V, const float* emb, const float* pe, float* ne_x, float* ne_part,
                            int32_t* ne_tok, const nd_beam_state* st, int32_t C, int32_t beam, int32_t n_best,
                            int32_t step, int32_t S, int32_t min_len, int32_t eos, const nd_classic_opts* opts,
                            void* stream) {
  if (!x || !ln_g || !ln_b || !gw || !gb || !emb || !ne_x || !ne_part || !classic_state_ok(st) ||
      !classic_opts_ok(opts) || C < 1 || S < 1 || step < 0 || step >= S || eos < 0 || (V >= 1 && eos >= V))
    return fail(ND_ERR_ARG, "beam_classic_step: bad arguments");
  const nd::BeamCall bc{.rows = {.C = C, .rpc = beam}, .n_best = n_best, .S = S, .min_len = min_len, .eos = eos};
  return status("beam_classic_step",
                nd::launch_beam_classic_step({.emb = emb, .pe = pe, .x = ne_x, .part = ne_part, .tok = ne_tok},
                                             {.x = x, .ln_g = ln_g, .ln_b = ln_b, .gw = gw, .gb = gb, .V = V},
                                             beam_state(*st), bc, step, classic_opts(*opts), (hipStream_t)stream));
}

int nd_op_beam_classic_finish(const nd_beam_state* st, int32_t C, int32_t beam, int32_t n_best, int32_t S,
                              const nd_classic_opts* opts, int32_t* tokens, float* scores, int32_t* lens,
                              void* stream) {
  if (!classic_state_ok(st) || !classic_opts_ok(opts) || !tokens || !scores || !lens || C < 1 || beam < 1 ||
      beam > 8 || n_best < 1 || S < 1)
    return fail(ND_ERR_ARG, "beam_classic_finish: bad arguments");
  return status("beam_classic_finish",
                nd::launch_beam_classic_finish(beam_state(*st), C, beam, n_best, S, classic_opts(*opts), tokens,
                                               scores, lens, (hipStream_t)stream));
}

int nd_op_attn_step_softmax(float* a, int64_t ld, const int32_t* span, int32_t R, int32_t rpc, int32_t T,
                            void* stream) {
  if (!a || !span || ld < T) return fail(ND_ERR_ARG, "attn_step_softmax: bad arguments");
  return status("attn_step_softmax", nd::launch_attn_step_softmax(a, (size_t)ld, span, R, rpc, T, (hipStream_t)stream));
}

int nd_op_beam_attn_gather(const nd_beam_state* st, int32_t C, int32_t n_best, int32_t S, int32_t max_len, int32_t T,
                           float* out, void* stream) {
  if (!st || !st->hyp_len || !st->hyp_anc || !out || C < 1 || n_best < 1 || S < 1 || max_len < 0 || T < 1)
    return fail(ND_ERR_ARG, "beam_attn_gather: bad arguments");
  return status("beam_attn_gather",
                nd::launch_beam_attn_gather(beam_state(*st), C, n_best, S, max_len, T, out, (hipStream_t)stream));
}
