/*
 * nanodec.h — C-ABI of libnanodec_hip.so, the MI355X (gfx950) engine for
 * NanoDecoder's translate path.
 *
 * The reference has no native boundary: its path is PyTorch modules driven by
 * translate/translator.py.  Each entry point below replaces the reference
 * interface named in its comment (file:line in achilles1989/NanoDecoder).
 * Plain pointers and sizes only; device pointers are HIP device memory owned
 * by the caller (PyTorch-ROCm tensors' data_ptr()).  Every function returns
 * 0 on success; on failure a nonzero ND_* code and a thread-local message in
 * nd_last_error().
 *
 * Threading: one context is bound to one device and must not be called
 * concurrently; every call sets the device first (the reference drives the
 * GPU from a multiprocessing.Pool result thread, translate.py:100-161).
 * All work is enqueued on the caller's stream; no hidden device-wide syncs.
 */
#ifndef NANODEC_H
#define NANODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ND_OK 0
#define ND_ERR_ARG 1      /* bad argument / shape / config */
#define ND_ERR_WEIGHT 2   /* unknown / missing / mis-shaped weight */
#define ND_ERR_HIP 3      /* HIP runtime error */
#define ND_ERR_STATE 4    /* call order (e.g. translate before finalize) */

#define ND_ENC_TRANSFORMER 0  /* encoder/transformer.py */
#define ND_ENC_NANO 1         /* encoder/nano_encoder.py (3x BiLSTM) */
#define ND_SELF_SCALED_DOT 0
#define ND_SELF_AVERAGE 1

typedef struct nd_ctx nd_ctx;

/* Architecture + capacity.  Mirrors the checkpoint ``opt`` the reference
 * builds its model from (models/model_builder.py:236-334). */
typedef struct nd_config {
  int32_t encoder_type;       /* ND_ENC_* */
  int32_t enc_layers;         /* 3 */
  int32_t dec_layers;         /* 3 */
  int32_t d_model;            /* 256 (only value compiled) */
  int32_t heads;              /* 8   (d_model / heads == 32) */
  int32_t d_ff;               /* 2048 (multiple of 128) */
  int32_t vocab;              /* |tgt vocab|, <= 32 */
  int32_t rnn_hidden;         /* 128 per direction (NanoEncoder) */
  int32_t position_encoding;  /* decoder sinusoidal PE (embeddings.py:36-43) */
  int32_t pad_idx, bos_idx, eos_idx;
  int32_t max_batch;          /* chunks per call */
  int32_t max_src_len;        /* 512 (src_seq_length) */
  int32_t max_steps;          /* max_length (100), at most 512 */
  int32_t max_beam;           /* beam_size upper bound (1 = greedy only) */
  int32_t device;             /* HIP device ordinal */
  int32_t self_attn_type;     /* decoder self-attention: ND_SELF_SCALED_DOT | ND_SELF_AVERAGE
                                 (decoder/transformer.py:33-37, onmt/modules/average_attn.py) */
} nd_config;

/* Replaces models/model_builder.py:load_test_model (:217-233) +
 * build_base_model (:236-382): allocate the engine for one device. */
int nd_create(const nd_config* cfg, nd_ctx** out);

/* Replaces model.load_state_dict (models/model_builder.py:356-357) for one
 * tensor.  ``name`` is the reference state-dict key (after the a_2/b_2 fix,
 * :345-353); generator keys are "generator.0.weight"/"generator.0.bias".
 * Unknown names and shape mismatches are errors (the reference's strict=False
 * silent fallback is deliberately NOT reproduced); decoder ``*.mask`` buffers
 * and BatchNorm ``num_batches_tracked`` are accepted and ignored. */
int nd_load_weight(nd_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);

/* Checks that every required weight was loaded and builds derived packed
 * weights.  Must be called once before any translate call.  The first call
 * also rebalances the decoder attentions' key / query and value / output
 * projections by exact powers of two per dimension (the model's function is
 * unchanged; a dimension far larger than the rest of its head would otherwise
 * cost the 24-bit K/V forms their bits); a weight loaded afterwards gets the
 * same scales. */
int nd_finalize(nd_ctx* ctx);

/* ctx (just created, no weight loaded, the same model configuration as src)
 * reads src's weights and every image nd_finalize derived from them instead
 * of holding its own; ctx is finalized by this call.  src must be finalized,
 * on the same device, and outlive ctx.  ND_ERR_STATE if a weight was loaded
 * into ctx; nd_load_weight on ctx afterwards returns ND_ERR_STATE.  ctx's own
 * raw weight buffers from nd_create stay allocated and unread.  For several contexts of one model on
 * one GPU (EnginePool lanes): one copy of the weights in the caches they
 * share (L2 per XCD, the Infinity Cache).  No reference counterpart (the
 * reference holds one model per process). */
int nd_share_weights(nd_ctx* ctx, const nd_ctx* src);

/* Greedy translate of a batch of chunks: encoder forward + max_len decoder
 * steps with argmax selection.  Replaces Translator.translate_batch ->
 * _translate_random_sampling (translate/translator.py:396-540) for
 * beam_size == 1 (keep_topk == 1): all max_len steps always run (no EOS
 * early exit, :455-483) and the score is the last step's top log-prob
 * (:491-499).
 *   d_signal  [B, T] f32 row-major, zero padded (make_nano, inputters/inputter.py:86-95)
 *   d_len     [B] i32 valid samples per chunk (src_lengths)
 *   d_span    [B] i32 padded length the reference batch would have had
 *             (= longest chunk of the reference batch; len <= span <= T).
 *             Positions >= span do not exist for that chunk.  1 <= span:
 *             the encoder's attention reads row span - 1 of the chunk.
 *   d_tokens  [B, max_len] i32 out;  d_score [B] f32 out
 *   d_logp    nullable [B, max_len, V] f32 out: per-step log-probs (pre min_len mask)
 *   stream    hipStream_t of the caller (void* here to keep HIP out of the ABI) */
int nd_translate_greedy(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                        int32_t B, int32_t T, int32_t max_len, int32_t min_len,
                        int32_t* d_tokens, float* d_score, float* d_logp, void* stream);

/* Greedy decode that also returns -attn_debug attention (translate/
 * translator.py:285-336, return_attention at :396-503): d_attn [B, max_len, T]
 * = per step the last decoder layer's context attention of head 0
 * (attn["std"], onmt/modules/multi_headed_attn.py:187-192) over source
 * positions t < span (zero beyond).  Otherwise as nd_translate_greedy. */
int nd_translate_greedy_attn(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                             int32_t B, int32_t T, int32_t max_len, int32_t min_len, int32_t* d_tokens, float* d_score,
                             float* d_logp, float* d_attn, void* stream);

/* Random sampling: Translator._translate_random_sampling with
 * sample_with_temperature (translate/translator.py:371-503).  Every step
 * draws the next token from softmax(log_probs / temp), restricted to the
 * keep_topk most likely tokens when keep_topk > 0 (the others set to -10000);
 * the score is the tempered (masked) value of the drawn token.  temp == 0 or
 * keep_topk == 1 is the argmax of nd_translate_greedy.  The draws come from a
 * counter-based generator keyed by (seed, chunk, step): equal seeds give
 * equal outputs (the reference draws from torch's global generator).
 * Outputs as nd_translate_greedy; d_attn nullable as nd_translate_greedy_attn. */
int nd_translate_sample(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
                        int32_t T, int32_t max_len, int32_t min_len, float temp, int32_t keep_topk, uint64_t seed,
                        int32_t* d_tokens, float* d_score, float* d_logp, float* d_attn, void* stream);

/* --fast beam search.  Replaces Translator._fast_translate_batch
 * (translate/translator.py:619-825) with GNMTGlobalScorer.alpha
 * (onmt/translate/beam.py:181-199; beta must be 0).  Per chunk the n_best
 * finished hypotheses, best first:
 *   d_tokens [B, n_best, max_len] i32 (EOS included when emitted; -1 padded)
 *   d_scores [B, n_best] f32, d_lens [B, n_best] i32
 *   d_steps  nullable [1] i32: decoder steps actually executed */
int nd_translate_beam(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                      int32_t B, int32_t T, int32_t beam, int32_t n_best, float alpha, int32_t max_len,
                      int32_t min_len, int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps,
                      void* stream);

/* Classic beam search: replaces Translator._translate_batch with the onmt
 * Beam (translate/translator.py:827-926, onmt/translate/beam.py:6-199; the
 * path the reference takes for beam_size > 1 without --fast).  d_group [B]
 * is the reference batch of every chunk (translate() batches batch_size
 * consecutive chunks of one read): a batch advances all its beams until each
 * is done, exactly as the reference loop does, however the chunks are packed
 * into this call.  length_penalty: 0 none, 1 wu, 2 avg (alpha for wu);
 * coverage penalty none.  Outputs as nd_translate_beam: tokens [B, n_best,
 * max_len] (-1 padded, EOS included when the hypothesis finished), scores
 * and lens [B, n_best]; d_steps (nullable) = steps run. */
int nd_translate_beam_classic(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                              const int32_t* d_group, int32_t B, int32_t T, int32_t beam, int32_t n_best,
                              int32_t length_penalty, float alpha, int32_t max_len, int32_t min_len,
                              int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, void* stream);

/* --fast beam search with -attn_debug (translate/translator.py:745-751,
 * :780-790): as nd_translate_beam, plus
 *   d_attn      [B, n_best, max_len, T] f32: row t of hypothesis k = the
 *               last layer's head-0 context attention of the decoder row
 *               that produced its token t (probabilities over keys < span,
 *               zero after), zero rows past the hypothesis length
 *   d_done_step [B] i32: the number of steps the chunk ran before it was
 *               dropped as finished (the caller derives the reference's
 *               memory_lengths[i] cut from the alive set of each step) */
int nd_translate_beam_attn(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                           int32_t B, int32_t T, int32_t beam, int32_t n_best, float alpha, int32_t max_len,
                           int32_t min_len, int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps,
                           float* d_attn, int32_t* d_done_step, void* stream);

/* Options of the classic onmt Beam (translate/translator.py:127-173,
 * onmt/translate/beam.py:6-243, onmt/translate/penalties.py). */
typedef struct nd_classic_opts {
  int32_t length_penalty;     /* 0 none, 1 wu, 2 avg */
  float alpha;                /* -alpha */
  float beta;                 /* -beta (coverage weight) */
  int32_t coverage_penalty;   /* 0 none, 1 wu, 2 summary */
  int32_t stepwise_penalty;   /* -stepwise_penalty */
  int32_t block_ngram_repeat; /* -block_ngram_repeat (0: off) */
  uint32_t ignore_mask;       /* -ignore_when_blocking: bit i = token id i */
} nd_classic_opts;

/* Classic beam search with the full option set: as nd_translate_beam_classic,
 * plus coverage penalties (wu / summary, at scoring time or stepwise) and
 * n-gram blocking, and optionally the hypotheses' attention.
 *   d_cut  [B] i32, required when coverage_penalty != 0: the attention length
 *          of the chunk's beams, memory_lengths[j] as the reference indexes
 *          its beam-tiled lengths (translate/translator.py:902-907)
 *   d_attn nullable [B, n_best, max_len, T] f32: as nd_translate_beam_attn
 * With coverage_penalty != 0 the attention is captured every step whether or
 * not d_attn is given. */
int nd_translate_beam_classic_ex(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                                 const int32_t* d_group, const int32_t* d_cut, int32_t B, int32_t T, int32_t beam,
                                 int32_t n_best, const nd_classic_opts* opts, int32_t max_len, int32_t min_len,
                                 int32_t* d_tokens, float* d_scores, int32_t* d_lens, int32_t* d_steps, float* d_attn,
                                 void* stream);

/* Teacher-forced scoring: replaces Translator._score_target (translate/translator.py:928-941): one
 * causally masked decoder pass over every position of every target, captured in one hipGraph.
 *   d_gold     [B, L] i32: the gold row of each chunk, tgt[1:] in the reference's terms:
 *              its tokens followed by EOS, then pad_idx
 *   d_gold_len [B] i32 in [1, L]: tokens counted, EOS included
 *   d_score    [B] f32: sum over i < gold_len of logp[i][gold[i]]
 *   d_tok_logp nullable [B, L] f32: the summands (0 at i >= gold_len)
 *   d_logp     nullable [B, L, V] f32: every position's log-probs (rows i >= gold_len unspecified)
 * L <= max_steps, B <= max_batch, T <= max_src_len (ND_ERR_ARG otherwise); an ND_SELF_AVERAGE decoder is
 * refused with ND_ERR_ARG (teacher-forced average attention is a cumulative mean, not built).  Token ids
 * outside [0, vocab) are clamped, never read out of bounds; the caller validates them.  The [B * L, .]
 * workspaces (and, on a context created with max_beam 1, the per-layer context K/V) are allocated by the
 * first call.  Honours nd_set_graphs, nd_set_exact_fp32 and nd_take_overflow like the translate calls. */
int nd_score_targets(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                     const int32_t* d_gold, const int32_t* d_gold_len, int32_t B, int32_t T, int32_t L,
                     float* d_score, float* d_tok_logp, float* d_logp, void* stream);

/* nd_score_targets that also returns where each target position looked (forced alignment, DESIGN.md
 * section 1.7): the same pass with the last decoder layer's context attention in its tapped form.
 *   d_attn [B, L, T] f32, required: row (b, i) = the head-0 probabilities of that attention at target
 *          position i, the quantity the translate calls return as attention; entries t >= min(span[b], T)
 *          are zero; rows i >= gold_len[b] are unspecified, as d_logp's are
 * Everything else is nd_score_targets: the outputs (bit for bit), the argument checks before the first HIP
 * call, the ND_SELF_AVERAGE refusal.  The attention buffer the translate_*_attn calls use is allocated by
 * the first call if the context has none; its own captured graph per (B, T, L).  nd_token_positions turns
 * d_attn (ld_chunk = L * T) into one signal sample per target position. */
int nd_score_targets_attn(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                          const int32_t* d_gold, const int32_t* d_gold_len, int32_t B, int32_t T, int32_t L,
                          float* d_score, float* d_tok_logp, float* d_logp, float* d_attn, void* stream);

/* Several candidate targets per chunk on one encoder pass (the reference has no such
 * call): "which of these K sequences does this signal support?"  The encoder and the context K/V
 * projections run once over the B chunks; the decoder runs over the B * K candidate rows, the K candidates
 * of a chunk being K * L consecutive query rows of its context attention.  nd_score_targets is the K = 1
 * case of the same function.
 *   d_cand     [B, K, L] i32: a gold row per (chunk, slot) exactly as nd_score_targets takes it: tokens,
 *              EOS, then pad_idx
 *   d_cand_len [B, K] i32 in [0, L], EOS included; 0 marks an empty slot (calls are rectangular: a chunk
 *              with fewer than K candidates leaves slots empty).  Values outside [0, L] are clamped on
 *              the device, token ids as in nd_score_targets
 *   d_score    [B, K] f32, required: the sum of the slot's token log-probabilities, nd_score_targets'
 *              quantity; -inf for an empty slot.  log P(y | x) is normalised over all sequences (EOS
 *              included), so the sums compare across candidates of different lengths
 *   d_post     nullable [B, K] f32: score - logsumexp over the chunk's non-empty slots; -inf for an empty slot
 *   d_best     nullable [B] i32: the non-empty slot with the largest score, the lowest slot on a tie; -1 when
 *              every slot is empty
 *   d_tok_logp nullable [B, K, L] f32, d_logp nullable [B, K, L, V] f32: as in nd_score_targets (tok_logp
 *              0 at i >= cand_len, logp rows there unspecified)
 * 1 <= K, B * K <= max_batch, L <= max_steps, T <= max_src_len (ND_ERR_ARG otherwise); an ND_SELF_AVERAGE
 * decoder is refused as by nd_score_targets; every check, null buffers included, comes before the first HIP
 * call.  Its own captured graph per (B, T, K, L).  Honours nd_set_graphs, nd_set_exact_fp32 and
 * nd_take_overflow like nd_score_targets, whose workspaces it uses.
 *
 * The posterior rule, one chunk per thread, slots in the order k = 0 .. K-1 (so a chunk's bits depend on its
 * own K scores only): m = the maximum over the non-empty slots, updated by s > m; sum = the sum of
 * expf(s_k - m) in slot order; post_k = (s_k - m) - logf(sum).  A NaN score is never best and makes the
 * chunk's post values NaN.  nd_cand_posterior applies the rule to given scores (no context needed; one
 * launch on `stream`): d_score [B, K] and d_cand_len [B, K] in, d_score_out [B, K] (required; may be d_score:
 * the scores with -inf in the empty slots), d_post (nullable) and d_best (nullable) out.  K < 1, B < 0 or a
 * null required buffer return ND_ERR_ARG before any HIP call; B == 0 returns ND_OK at once. */
int nd_score_candidates(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span,
                        const int32_t* d_cand, const int32_t* d_cand_len, int32_t B, int32_t T, int32_t K, int32_t L,
                        float* d_score, float* d_post, int32_t* d_best, float* d_tok_logp, float* d_logp,
                        void* stream);
int nd_cand_posterior(const float* d_score, const int32_t* d_cand_len, int32_t B, int32_t K, float* d_score_out,
                      float* d_post, int32_t* d_best, void* stream);

/* Signal front end (utils/labelop.py:194-243, extract_fast5_raw): R raw
 * reads concatenated in d_raw (float64, read r at d_offsets[r] ..
 * d_offsets[r+1]) normalised per read into d_out (float32, same offsets).
 * method: 0 none, 1 median (x - median) / MAD with statsmodels' robust.mad
 * (median(|x - median| / 0.6744897501960817)), 2 mean ((x - median) / std,
 * as the reference centres it).  fp64 arithmetic and exact medians, so the
 * float32 chunks equal the reference's (method 2: within 1 ulp, the std is a
 * reduction).  No context needed. */
int nd_normalize_reads(const double* d_raw, const int64_t* d_offsets, int32_t R, int32_t method, float* d_out,
                       void* stream);

/* Windowing (utils/labelop.py:225-233) straight into a signal batch: chunk c
 * = d_len[c] samples of read d_read[c] from d_start[c], zero padded to T, is
 * row c of d_signal [C, T].  The caller lists the windows (stride, length). */
int nd_window_reads(const float* d_sig, const int64_t* d_offsets, const int32_t* d_read, const int32_t* d_start,
                    const int32_t* d_len, int32_t C, int32_t T, float* d_signal, void* stream);

/* Read assembly (utils/labelop.py:310-352, add_count / simple_assembly with
 * flag_intersection, and the argmax + index2base of translate.py:84-87) for a
 * group of R reads in one call.  d_bases [total_bases] u8: every chunk's best
 * hypothesis as ASCII with the spaces removed, concatenated; chunk c is
 * d_chunk_off[c] .. d_chunk_off[c+1] (C + 1 offsets, empty chunks allowed and
 * skipped as the reference drops them), read r owns the consecutive chunks
 * d_read_off[r] .. d_read_off[r+1] (R + 1 offsets).  Consecutive non-empty
 * chunks are aligned by their longest common substring (the longest, then the
 * earliest in the first chunk, then the earliest in the second; no shared
 * character: displacement la - lb), exactly difflib's longest matching block
 * while the second chunk has fewer than 200 chars; the chunks vote per column
 * and class (A C G T M, case folded) and the column's call is the class with
 * the most votes, the lowest on a tie.
 *   d_seq     [total_bases] u8: read r's bases start at byte
 *             d_chunk_off[d_read_off[r]] (a consensus is never longer than the
 *             sum of its chunks); bytes past a read's length are 0
 *   d_seq_len [R] i32: bases of read r, or -1 when d_status[r] != 0
 *   d_status  [R] i32: 0 = assembled.  Bit 0: some chunk has 200 or more
 *             chars (difflib's autojunk heuristic starts there and changes the
 *             block found; that regime is not reproduced).  Bit 1: some char's
 *             upper case is not one of A C G T M.  The caller assembles such a
 *             read on the host.
 * d_work holds nd_assemble_reads_work_bytes(C, total_bases) bytes.  Null
 * buffers, negative sizes, total_bases >= 2^31 or a smaller work_bytes return
 * ND_ERR_ARG before any HIP call; R == 0 returns ND_OK at once.  Everything is
 * enqueued on `stream`: no allocation, no synchronisation.  No context needed. */
int64_t nd_assemble_reads_work_bytes(int32_t C, int64_t total_bases);
int nd_assemble_reads(const uint8_t* d_bases, const int32_t* d_chunk_off, const int32_t* d_read_off, int32_t R,
                      int32_t C, int64_t total_bases, uint8_t* d_seq, int32_t* d_seq_len, int32_t* d_status,
                      void* d_work, int64_t work_bytes, void* stream);

/* Per-base qualities (FASTQ).  The reference writes no qualities; these three
 * entry points carry the model's own probability of each called token through
 * the assembly vote.  No context needed.
 *
 * Token weight of a token with log-probability lp (fp32):
 *   w = min(65535, floor(65535 * exp((double)lp) + 0.5)), a uint16; 0 for a
 *   non-finite lp or a token id outside [0, V) (the beam's -1 padding).
 * nd_token_weights writes d_w [B, S] from d_tokens [B, S] and exactly one of
 *   d_logp     [B, S, V] f32: lp = d_logp[b][s][d_tokens[b][s]]
 *   d_tok_logp [B, S]    f32: lp = d_tok_logp[b][s]
 * in one launch on `stream`, with no allocation and no synchronisation.
 * Negative sizes, V < 1, B * S >= 2^31, a null buffer, or neither or both of
 * the two log-prob inputs return ND_ERR_ARG before any HIP call.
 *
 * Column quality of one column of a read's vote: n = its votes of all classes,
 * S = the sum of the weights of the votes for the winning class (the winner
 * exactly as nd_assemble_reads picks it), E = 65535 n - S; Q is the largest k
 * in 0..40 with (double)E * RATIO[k] <= (double)(65535 n), RATIO[k] the double
 * 10.0 ** (k / 10.0); Q = 0 when n = 0.  nd_phred_ratios copies the first
 * n <= 41 entries of RATIO out (ND_ERR_ARG for a null out or another n).
 *
 * nd_assemble_reads_q is nd_assemble_reads with
 *   d_qw   [total_bases] u16 (in):  the weight of each byte of d_bases
 *   d_qual [total_bases] u8  (out): Q of the columns of the assembled reads,
 *          laid out like d_seq; 0 past a read's length
 * Overlap, placement, d_seq, d_seq_len and d_status are those of
 * nd_assemble_reads on the same input; the weight sums are 64-bit integers,
 * so the bytes do not depend on the order the votes arrive in.  d_work holds
 * nd_assemble_reads_q_work_bytes(C, total_bases) bytes (nd_assemble_reads' plus
 * 5 * total_bases * 8); argument checks and the R == 0 and C == 0 paths as
 * nd_assemble_reads. */
int nd_token_weights(const int32_t* d_tokens, const float* d_logp, const float* d_tok_logp, int32_t B, int32_t S,
                     int32_t V, uint16_t* d_w, void* stream);
int nd_phred_ratios(double* out, int32_t n);
int64_t nd_assemble_reads_q_work_bytes(int32_t C, int64_t total_bases);
int nd_assemble_reads_q(const uint8_t* d_bases, const uint16_t* d_qw, const int32_t* d_chunk_off,
                        const int32_t* d_read_off, int32_t R, int32_t C, int64_t total_bases, uint8_t* d_seq,
                        uint8_t* d_qual, int32_t* d_seq_len, int32_t* d_status, void* d_work, int64_t work_bytes,
                        void* stream);

/* Per-base methylation probabilities (CpG models: a vocabulary with the tokens
 * "C" and "M", M a methylated C).  The reference writes the hard letter M
 * only; these three entry points carry P(methylated | the base is a C) from
 * the calls' log-probs through the assembly vote, beside the quality.  No
 * context needed.
 *
 * Token modification weight of token t with that step's log-probs lp (fp32),
 * canon_id the id of "C" and mod_id the id of "M":
 *   t not in {canon_id, mod_id} (the beam's -1 padding included): mw = 0;
 *   else d = (double)lp[canon_id] - (double)lp[mod_id], p = 1 / (1 + exp(d)),
 *   mw = min(65535, floor(65535 * p + 0.5)), a uint16, every operation in
 *   double and rounded once (no FMA); d = +inf gives 0, d = -inf 65535; a NaN
 *   d falls back to the hard call: 65535 when t == mod_id, else 0.
 * nd_token_mod_weights writes d_mw [B, S] from d_tokens [B, S] and d_logp
 * [B, S, V] in one launch on `stream`, with no allocation and no
 * synchronisation.  Negative sizes, V < 1, B * S >= 2^31, an id outside
 * [0, V), canon_id == mod_id or a null buffer return ND_ERR_ARG before any
 * HIP call.
 *
 * Column value of one column of a read's vote: n_cm = its votes of class C
 * plus those of class M, W = the sum of mw over exactly those votes (a 64-bit
 * unsigned integer, so the bytes do not depend on the order the votes arrive
 * in).  A column whose call (exactly as nd_assemble_reads makes it) is C or M
 * is a site: ML = min(255, (256 * W) div (65535 * n_cm)), integer division
 * (n_cm >= 1 there), SAM's ML scale.  Every other column gets 0.  The call
 * itself is never changed: a column called C may carry ML >= 128 (a 1:1 tie
 * of a C vote and a confident M vote goes to the lower class, C).
 *
 * nd_assemble_reads_m is nd_assemble_reads_q with
 *   d_mw [total_bases] u16 (in):  the modification weight of each byte of
 *        d_bases (every char of a token's word carries the token's)
 *   d_ml [total_bases] u8  (out): ML of the columns of the assembled reads,
 *        laid out like d_seq; 0 off-site and past a read's length
 * d_seq, d_qual, d_seq_len and d_status are those of nd_assemble_reads_q on
 * the same input.  d_work holds nd_assemble_reads_m_work_bytes(C, total_bases)
 * bytes (nd_assemble_reads_q's plus total_bases * 8); argument checks and the
 * R == 0 and C == 0 paths as nd_assemble_reads. */
int nd_token_mod_weights(const int32_t* d_tokens, const float* d_logp, int32_t B, int32_t S, int32_t V,
                         int32_t canon_id, int32_t mod_id, uint16_t* d_mw, void* stream);
int64_t nd_assemble_reads_m_work_bytes(int32_t C, int64_t total_bases);
int nd_assemble_reads_m(const uint8_t* d_bases, const uint16_t* d_qw, const uint16_t* d_mw,
                        const int32_t* d_chunk_off, const int32_t* d_read_off, int32_t R, int32_t C,
                        int64_t total_bases, uint8_t* d_seq, uint8_t* d_qual, uint8_t* d_ml, int32_t* d_seq_len,
                        int32_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* Per-base signal positions.  The reference has no such output; these three
 * entry points turn the last decoder layer's head-0 context attention (what
 * nd_translate_greedy_attn, nd_translate_sample, nd_translate_beam_attn and
 * nd_translate_beam_classic_ex return in d_attn) into one sample index per
 * token and carry it through the assembly vote.  Integers throughout, so the
 * values do not depend on the order of any sum.  No context needed.
 *
 * Token position of one attention row a[0..T) (fp32) of a chunk with span sp:
 * only t < min(sp, T) is read.  q_t = 0 when !(a[t] > 0) (NaN, negatives and
 * -0), 2^24 when a[t] >= 1, else floor((double)a[t] * 16777216.0 + 0.5)
 * (exact in fp64).  Q = sum q_t and M = sum q_t * t in 64-bit unsigned
 * integers; c = (2 M + Q) div (2 Q), the centroid rounded half up, c = 0 when
 * Q == 0.  Per chunk the positions are made monotone over the steps:
 * m[0] = c[0], m[s] = max(m[s-1], c[s]); a zero row keeps the position before
 * it.
 * nd_token_positions writes d_pos [B, S] i32 = m from d_span [B] and d_attn:
 * row s of chunk b is at d_attn + b * ld_chunk + s * T (the greedy and
 * sampling output [B, max_len, T]: ld_chunk = max_len * T; the beam output
 * [B, n_best, max_len, T]: ld_chunk = n_best * max_len * T, which selects
 * hypothesis 0, whose rows past its length are zero rows).  One launch on
 * `stream`, no allocation, no synchronisation.  Negative sizes, T < 1,
 * T > 2^19 (2 M + Q then stays inside 64 bits whatever a row holds),
 * ld_chunk < S * T, B * S >= 2^31 or a null buffer return ND_ERR_ARG before
 * any HIP call.
 *
 * Every char of a token's word carries the token's m; the absolute position
 * of a char of chunk ci of a read (its index among all of the read's chunks,
 * empty ones included) is ci * src_seq_stride + m, a uint32.
 *
 * Column position of one column of a read's vote: n = its votes of all
 * classes (exactly the votes nd_assemble_reads counts, those that lost the
 * call included), P = the 64-bit sum of their absolute positions; the column
 * gets P div n, and 0 when n = 0.  Read positions are the running maximum of
 * the column positions along the read: r[0] = col[0], r[x] = max(r[x-1],
 * col[x]).
 *
 * nd_assemble_reads_p is nd_assemble_reads with
 *   d_bp   [total_bases] u32 (in):  the absolute position of each byte of
 *          d_bases
 *   d_rpos [total_bases] u32 (out): the read positions of the assembled
 *          reads, laid out like d_seq; 0 past a read's length
 * Overlap, placement, d_seq, d_seq_len and d_status are those of
 * nd_assemble_reads on the same input.  d_work holds
 * nd_assemble_reads_p_work_bytes(C, total_bases) bytes (nd_assemble_reads'
 * plus total_bases * 8); argument checks and the R == 0 and C == 0 paths as
 * nd_assemble_reads.  One more launch than nd_assemble_reads: the per-read
 * running maximum, in blocks of 256 columns with a carry. */
int nd_token_positions(const float* d_attn, int64_t ld_chunk, const int32_t* d_span, int32_t B, int32_t S, int32_t T,
                       int32_t* d_pos, void* stream);
int64_t nd_assemble_reads_p_work_bytes(int32_t C, int64_t total_bases);
int nd_assemble_reads_p(const uint8_t* d_bases, const uint32_t* d_bp, const int32_t* d_chunk_off,
                        const int32_t* d_read_off, int32_t R, int32_t C, int64_t total_bases, uint8_t* d_seq,
                        uint32_t* d_rpos, int32_t* d_seq_len, int32_t* d_status, void* d_work, int64_t work_bytes,
                        void* stream);

/* Read accuracy against known sequences: the global alignment of P called
 * reads to their truths in one call.  The reference measures this outside its
 * own code (minimap2, then matches over alignment length); no reference
 * equivalent.  No context needed.
 *
 * The rule.  Call a[0..n), truth b[0..m), bytes compared for equality (the
 * caller normalises them: upper case, M written as C on both sides).
 *   D[i][0] = i, D[0][j] = j,
 *   D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1).
 * Direction at (i, j), taken in this order: diagonal if i, j >= 1 and
 * D[i-1][j-1] + (a[i-1] != b[j-1]) == D[i][j]; else up if i >= 1 and (j == 0
 * or D[i-1][j] + 1 == D[i][j]), which consumes a[i-1] only (an inserted base in
 * the call); else left, which consumes b[j-1] only (a base missing from the
 * call).  The alignment is the path those directions give from (n, m) back to
 * (0, 0).
 *   d_call, d_truth [bytes] u8 and d_call_off, d_truth_off [P + 1] i32: pair p
 *             is d_call[d_call_off[p] .. d_call_off[p+1]) against the same
 *             slice of d_truth; empty sides are legal (all insertions, or all
 *             deletions)
 *   d_counts  [P, 5] i32: {dist, n_match, n_sub, n_ins, n_del} with
 *             n_match + n_sub + n_ins == n, n_match + n_sub + n_del == m and
 *             dist == n_sub + n_ins + n_del; five times -1 when d_status[p] != 0
 *   d_ops     [d_call_off[P]] u8, may be null: per call base, laid out like
 *             d_call, 0 = match, 1 = mismatch, 2 = insertion; 0 for the bases
 *             of a pair whose d_status is not 0
 *   d_status  [P] i32: 0 = aligned.  Bit 0: n or m above 8192 (distances to
 *             16384 fit 16 bits; the caller aligns a longer read on the host).
 *             Bit 1: the pair's directions did not fit into d_work because
 *             `cells` was understated.
 * `cells` is the caller's sum of n * m over the pairs within the cap (an
 * over-estimate is fine).  d_work (8-byte aligned) holds the pairs' 64-bit
 * offsets, derived on the device, and their packed 2-bit directions; its
 * layout is internal.  nd_align_seqs_work_bytes(P, cells) = cells / 4 + 16 P +
 * 64 is the bound for it (-1 for a negative argument); which pairs fit depends
 * on `cells` alone, not on a larger work_bytes.  Integer min-plus throughout:
 * the results do not depend on the grid, the order of the pairs or the stream.
 * P == 0 returns ND_OK at once; a negative P or cells, a work_bytes below the
 * bound, a null buffer other than d_ops or a misaligned d_work return
 * ND_ERR_ARG before any HIP call.  Two launches on `stream`: no allocation, no
 * synchronisation. */
int64_t nd_align_seqs_work_bytes(int32_t P, int64_t cells);
int nd_align_seqs(const uint8_t* d_call, const int32_t* d_call_off, const uint8_t* d_truth,
                  const int32_t* d_truth_off, int32_t P, int64_t cells, int32_t* d_counts, uint8_t* d_ops,
                  int32_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* Read accuracy against a shared reference (a genome, a control sequence):
 * where each of P segments of called reads lies in it and on which strand
 * (nd_locate_segs), then the alignment of each segment to the window found,
 * with free ends on the reference side (nd_align_fit).  The reference maps its
 * reads outside its own code (pipeline.evaluate.sh: minimap2); no reference
 * equivalent.  No context needed.  Integers throughout: the results do not
 * depend on the grid, the order of the segments or the stream, and equal the
 * host rule of nanodecoder_amd/accuracy.py (locate_host, fit_host).
 *
 * The reference is R records concatenated with no separator, d_rec_off [R + 1]
 * i32 their starts (d_rec_off[R] = the total, at most 2^23).  Base codes A, C,
 * G, T = 0..3, any other byte invalid.  A k-mer is 15 consecutive valid bases
 * inside one record, its code the 30-bit number with the first base in the
 * highest bits.  The index is (code, pos) of every k-mer of the forward
 * reference sorted by code, then pos, without the codes that occur more than 8
 * times: d_idx_code, d_idx_pos [idx_len] u32.
 *
 * nd_locate_segs.  Segment p is d_call[d_call_off[p] .. d_call_off[p+1]), n
 * bases.  For strand 0 (the segment) and strand 1 (its reverse complement;
 * invalid bytes stay as they are): every k-mer of the query at offset x and
 * every index entry (code, y) with its code gives one vote to bin
 * (y - x + 4096) >> 9; score[b] = votes[b] + votes[b + 1]; the hit is the
 * (strand, b) with the largest score, strand 0 before strand 1, then the
 * lowest b.  With lo = (b << 9) - 4096 the window is that of the record
 * containing clamp(lo + 512 + n / 2, 0, total - 1): w0 = max(record start,
 * lo - 1024), w1 = min(record end, lo + 1024 + n + 1024), so w1 - w0 <= n +
 * 3072.
 *   d_hit     [P, 4] i32: {strand, w0, w1, votes = the hit's score}; w0 = w1 =
 *             0 for an unmapped segment
 *   d_status  [P] i32: 0 = mapped; bit 0 = unmapped: a score below 8, n below
 *             15 or above 4096, or a total above 2^23
 *   d_call_or [d_call_off[P]] u8: the oriented segments, laid out like d_call
 *             (the reverse complement for strand 1); must not be d_call
 * One workgroup per segment, one launch on `stream`: no allocation, no
 * synchronisation.  P == 0 returns ND_OK at once; a negative P, idx_len or R or
 * a null buffer (the index arrays may be null when idx_len == 0) return
 * ND_ERR_ARG before any HIP call.
 *
 * nd_align_fit.  Pair p is d_call_or[d_call_off[p] .. d_call_off[p+1]) = a[0..n)
 * against the window b[0..m) = d_ref[d_hit[p][1] .. d_hit[p][2]) of the whole
 * reference d_ref [ref_len] u8.  Borders D[0][j] = 0, D[i][0] = i; recurrence
 * and direction order as nd_align_seqs; j* is the smallest j in 0..m with
 * D[n][j] minimal; the path runs from (n, j*) until i == 0, nothing consumed
 * on row 0, and at j == 0 with i > 0 the rest is insertions.
 *   d_counts  [P, 5] i32: {dist = D[n][j*], n_match, n_sub, n_ins, n_del},
 *             n_match + n_sub + n_ins == n, n_match + n_sub + n_del == the
 *             span's length; five times -1 when d_status[p] != 0
 *   d_span    [P, 2] i32: the aligned interval of d_ref, {w0 + t_start, w0 +
 *             j*}; twice -1 when d_status[p] != 0
 *   d_ops     [d_call_off[P]] u8, may be null: per oriented call base, 0 =
 *             match, 1 = mismatch, 2 = insertion; 0 when d_status[p] != 0
 *   d_status  [P] i32, read and written: a pair that comes in with bit 0 set
 *             (unmapped) is skipped and keeps its status; otherwise 0 =
 *             aligned, bit 1 = the pair's directions did not fit because
 *             `cells` was understated, bit 2 = n or m above 8192 or a window
 *             outside [0, ref_len]
 * `cells` is the caller's bound on the sum of n * m over the pairs aligned
 * (the sum of n * (n + 3072) holds after nd_locate_segs); d_work and
 * nd_align_fit_work_bytes are as for nd_align_seqs, and so are the argument
 * errors.  Two launches on `stream`; after nd_locate_segs on the same stream
 * no host round trip is needed in between. */
int nd_locate_segs(const uint8_t* d_call, const int32_t* d_call_off, int32_t P, const uint32_t* d_idx_code,
                   const uint32_t* d_idx_pos, int32_t idx_len, const int32_t* d_rec_off, int32_t R, int32_t* d_hit,
                   int32_t* d_status, uint8_t* d_call_or, void* stream);
int64_t nd_align_fit_work_bytes(int32_t P, int64_t cells);
int nd_align_fit(const uint8_t* d_call_or, const int32_t* d_call_off, const uint8_t* d_ref, int32_t ref_len,
                 const int32_t* d_hit, int32_t P, int64_t cells, int32_t* d_counts, int32_t* d_span, uint8_t* d_ops,
                 int32_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* Consensus of the mapped reads: the alignment above with the reference
 * position of every call base kept (nd_align_fit_pos), the pile of all pairs on
 * the reference (nd_pileup_add), and the call of a consensus base per position
 * (nd_pileup_call).  The reference evaluates its consensus outside its own code
 * (scripts/analysis.sh); no reference equivalent.  No context needed.  Integers
 * throughout: the results do not depend on the grid, the order of the pairs or
 * the stream, and equal the host rule of nanodecoder_amd/accuracy.py
 * (fit_pos_host, pile_add_host, consensus_host).
 *
 * nd_align_fit_pos is nd_align_fit with one more output; every other output is
 * bit for bit nd_align_fit's.
 *   d_rpos    [d_call_off[P]] i32, laid out like d_ops: for oriented call base
 *             i the position in d_ref it sits on.  A diagonal step at cell
 *             (i + 1, j): w0 + j - 1, the base it is matched or mismatched to;
 *             an up step (an insertion) at column j: w0 + j - 1, the base to
 *             its left, w0 - 1 on the column-0 border; -1 for every base of a
 *             pair whose d_status[p] != 0
 * The deleted reference bases are the positions of the span that no diagonal
 * step took; they lie strictly between two diagonal steps of the pair.
 * nd_align_fit_pos_work_bytes equals nd_align_fit_work_bytes; statuses and
 * argument errors are nd_align_fit's, and a null d_rpos is ND_ERR_ARG.
 *
 * nd_pileup_add.  d_pile [9, ref_len] u32, plane by plane: A, C, G, T, D, iA,
 * iC, iG, iT.  A base with op 0 or 1 is a diagonal base.  Every pair with
 * d_status[p] == 0 adds:
 *   a diagonal base: +1 in the plane of its code at its rpos; a call byte other
 *     than A, C, G, T adds nothing;
 *   deleted positions: +1 in D at every position strictly between the rpos of
 *     two consecutive diagonal bases of the pair;
 *   an insertion run with a diagonal base of the pair on both sides: +1 in the
 *     i plane of the run's first base (if it is A, C, G or T), at the rpos of
 *     the diagonal base before it.  Leading and trailing insertions are not
 *     piled, and a longer insertion is named by its first base only.
 * A position outside [0, ref_len) is skipped wherever it would add.  The table
 * accumulates over calls; the caller zeroes it once.  One thread per call base,
 * unsigned integer atomics, one launch on `stream`: no allocation, no
 * synchronisation.  P == 0 or ref_len == 0 returns ND_OK at once; a negative P
 * or ref_len or a null buffer return ND_ERR_ARG before any HIP call.
 *
 * nd_pileup_call.  At position r, cov = A + C + G + T + D.
 *   d_cons    [ref_len] u8: 255 when cov < min_cov (uncalled); otherwise the
 *             index 0..4 (4 = deleted) of the largest of the five counts, the
 *             lowest index on a tie
 *   d_ins     [ref_len] u8: when r is called and 2 (iA + iC + iG + iT) > cov,
 *             the index 0..3 of the largest of the four i counts, the lowest on
 *             a tie: an inserted base after r; otherwise 255
 *   d_cov     [ref_len] i32: cov
 *   d_rec     [R, 6] i64, zeroed by the call itself: per record of d_rec_off
 *             [R + 1] the sums over its positions {called, match, sub, del,
 *             ins, cov_sum}: match = cons is the code of d_ref[r]; sub = cons <
 *             4 and is not (a reference byte other than A, C, G, T counts as
 *             sub); del = cons == 4; ins = the called insertions; cov_sum = cov
 *             over the called positions
 * Consensus identity is match / (match + sub + del + ins).  A memset and one
 * launch on `stream`: sums per workgroup first, then one 64-bit atomic per
 * workgroup, record touched and sum; no allocation, no synchronisation.  R == 0
 * or ref_len == 0 returns ND_OK at once; min_cov < 1, a negative size or a null
 * buffer return ND_ERR_ARG before any HIP call. */
int64_t nd_align_fit_pos_work_bytes(int32_t P, int64_t cells);
int nd_align_fit_pos(const uint8_t* d_call_or, const int32_t* d_call_off, const uint8_t* d_ref, int32_t ref_len,
                     const int32_t* d_hit, int32_t P, int64_t cells, int32_t* d_counts, int32_t* d_span,
                     uint8_t* d_ops, int32_t* d_rpos, int32_t* d_status, void* d_work, int64_t work_bytes,
                     void* stream);
int nd_pileup_add(const uint8_t* d_call_or, const int32_t* d_call_off, const uint8_t* d_ops, const int32_t* d_rpos,
                  const int32_t* d_status, int32_t P, uint32_t* d_pile, int32_t ref_len, void* stream);
int nd_pileup_call(const uint32_t* d_pile, const uint8_t* d_ref, int32_t ref_len, const int32_t* d_rec_off, int32_t R,
                   int32_t min_cov, uint8_t* d_cons, uint8_t* d_ins, int32_t* d_cov, int64_t* d_rec, void* stream);

/* Encoder forward only; writes the memory bank [B, T, d_model] (rows
 * t >= span are unspecified).  Replaces Translator._run_encoder
 * (translate/translator.py:542-559).  Used by parity tests. */
int nd_encode(nd_ctx* ctx, const float* d_signal, const int32_t* d_len, const int32_t* d_span, int32_t B,
              int32_t T, float* d_memory, void* stream);

/* The context's own HIP stream (non-blocking; the translate graphs run on
 * it).  A caller that enqueues its inputs and reads
 * its outputs on this stream needs no cross-stream join per call. */
void* nd_stream(nd_ctx* ctx);

/* Enables/disables hipGraph capture of the translate calls (default on). */
int nd_set_graphs(nd_ctx* ctx, int enable);

/* Context-attention form: 0 (default) = the memory-bank form for greedy
 * decoding (ctx K/V projections folded into the query / output GEMMs, one
 * shared 256-float memory row per source position) and the per-layer K/V
 * form for beam search; 1 = the K/V form always.  Same results to fp32
 * rounding; replaces decoder/transformer.py:82-86 + multi_headed_attn.py:
 * 142-177's context path. */
int nd_set_ctx_path(nd_ctx* ctx, int path);

/* Arithmetic of the products: 0 (default) = split-fp16 (each fp32 operand as
 * an fp16 hi/lo pair, 22 significant bits, three fp16 MFMA products summed in
 * fp32 accumulators); 1 = exact fp32 (fp32-MFMA kernels for every GEMM, the
 * encoder attention and the BiLSTM recurrence), the reference's own fp32
 * arithmetic (nn.Linear / bmm in fp32).  Off when a context is created.  The
 * captured graphs of both forms are kept (keyed by it). */
int nd_set_exact_fp32(nd_ctx* ctx, int enable);

/* Cache policy of the greedy memory bank: nontemporal != 0 streams it with
 * non-temporal loads (it then does not stay in the Infinity Cache).  For
 * several contexts on one GPU (EnginePool) whose banks together exceed the
 * cache.  Default 0.  No reference counterpart. */
int nd_set_bank_policy(nd_ctx* ctx, int nontemporal);

/* Workgroups of the greedy memory-bank kernel at most: 0 (default) = one per
 * chunk, i.e. every CU while it streams; n > 0 = n workgroups walking the
 * chunks.  The kernel holds 137 KB of a CU's 160 KB LDS, so while it runs no
 * other context's LDS-staged GEMM fits beside it; EnginePool lanes cap it at
 * half the CUs (measured, 3 lanes x 256 chunks: 18.3 -> 17.6 ms per call).
 * Same results (each chunk is one workgroup's work either way).  No reference
 * counterpart. */
int nd_set_bank_grid(nd_ctx* ctx, int32_t workgroups);

/* The decoder step's K = 2048 products (W_vo, FFN2 at 256 rows) split over
 * workgroups (gemm_p16k_kernel, partial slabs + arrival tickets) instead of
 * one workgroup per output tile.  Default 0 (off): a lone call is faster
 * without; several calls in flight (EnginePool lanes) gain from it (DESIGN.md
 * section 3).  Results differ from the unsplit kernel's in fp32 rounding of
 * the K sum only.  No reference counterpart. */
int nd_set_gemm_splitk(nd_ctx* ctx, int32_t on);

/* Split-fp16 range guard.  An activation operand the split form carries as
 * fp16 hi/lo leaves the fp16 range from |x| = 65504 on, where the
 * reference's fp32 arithmetic is still finite.  Every kernel that splits an
 * activation it does not normalise itself (GEMMs without a LayerNorm
 * prologue, the encoder attention's Q/K/V) raises the context's overflow
 * word when it sees one.  nd_take_overflow enqueues, on `stream`, a copy of
 * that word to d_out (one int32: nonzero = some product of the calls
 * enqueued since the last take saw an out-of-range operand) and clears it.
 * Call it right after each translate call, as the Python Translator does,
 * and rerun a flagged call after nd_set_exact_fp32(ctx, 1).  No reference
 * counterpart: the reference computes in fp32 (nn.Linear / bmm). */
int nd_take_overflow(nd_ctx* ctx, int32_t* d_out, void* stream);

/* Launch-duration stamps of the decoder's context attention (the bench's
 * roofline kernel: dec_mem_attention_kernel for greedy, dec_ctx_attention_kernel
 * for beam), taken inside the kernels with the constant-rate wall clock while
 * enable != 0 (part of the captured graphs, so they time graph replays).
 * nd_kernel_stamps waits for the context's stream and returns the mean
 * duration (first workgroup start to last workgroup end) of the launches of
 * the last call. */
int nd_set_kernel_stamps(nd_ctx* c, int enable);
int nd_kernel_stamps(nd_ctx* c, float* avg_us, int32_t* launches);

/* Kernel statistics of the last translate call (ms of device time per
 * phase, measured with HIP events on the engine stream when enabled).  The
 * scoring calls report too: a timed one runs its launches as two pieces, the
 * encoder with the context K/V projections, then the decoder rows. */
int nd_set_timing(nd_ctx* ctx, int enable);
int nd_last_timing(nd_ctx* ctx, float* encode_ms, float* decode_ms);

void nd_destroy(nd_ctx* ctx);
const char* nd_last_error(void);
const char* nd_version(void);

/* ---- diagnostics (no reference counterpart) ----------------------------- */

/* GEMM kernel routes, counted per process each time a GEMM is enqueued (a
 * graph capture enqueues once; replays are not counted).  Lets a test check
 * which kernels a workload of a given size runs (gemm.hip launch_gemm_p16 /
 * launch_gemm pick the kernel from M, N, K). */
#define ND_ROUTE_P16_SMALL 0   /* gemm_p16_kernel<1,4,64>  (K = 256, few row blocks) */
#define ND_ROUTE_P16_N64 1     /* retired, always 0: no shape reached its kernel (the index is kept) */
#define ND_ROUTE_P16_LN128 2   /* retired, always 0 (likewise) */
#define ND_ROUTE_P16S_2X4 3    /* gemm_p16s_kernel<2,4>    (K = 256, LDS-staged, 32-row blocks) */
#define ND_ROUTE_P16S_2X2 4    /* gemm_p16s_kernel<2,2> */
#define ND_ROUTE_P16_LONGK 5   /* gemm_p16_kernel<1,8,*>   (K = 512 / 1024 / 2048) */
#define ND_ROUTE_P16_BIG 6     /* P16 operands on the LDS-tiled row-major kernel (large M) */
#define ND_ROUTE_TILE256 7     /* gemm_f32_kernel 256x256 tiles */
#define ND_ROUTE_TILE128 8     /* gemm_f32_kernel 128x128 tiles */
#define ND_ROUTE_TILE64 9      /* gemm_f32_kernel 64x64 tiles */
#define ND_ROUTE_P16_SPLITK 10 /* gemm_p16k_kernel (K = 1024 / 2048, 32 x 32 tiles split over K, 128 < M) */
#define ND_ROUTE_N 11
/* counts[0 .. min(n, ND_ROUTE_N) - 1] <- launches per route since the last
 * reset; reset != 0 zeroes the counters afterwards. */
int nd_gemm_routes(int64_t* counts, int32_t n, int32_t reset);

/* The library's run-time switches (ND_* environment variables read by the
 * kernels' launchers, A/B timing knobs): writes "NAME=value" pairs separated
 * by ';' for every switch whose environment value differs from its default
 * into buf (NUL-terminated, truncated to len) and returns their number. */
int nd_switches(char* buf, int32_t len);

/* ---- op-level entry points (unit tests of individual kernels) ---------- */

/* C[M,N] = epilogue(prologue(A)[M,K] . W[N,K]^T + bias):
 * prologue row normalisation (A - mean) / sqrt(var + 1e-6) over K when
 * norm != 0 (a LayerNorm whose affine was folded into W / bias by
 * nd_op_fold_layernorm); relu when relu != 0; + R[M,N] when R != NULL.
 * All fp32, row-major, dense.  Replaces nn.Linear (+ the LayerNorm before it):
 * onmt/modules/multi_headed_attn.py:155-157, onmt/modules/position_ffn.py:38-40,
 * decoder/transformer.py:75,88, encoder/transformer.py:50. */
int nd_op_gemm(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M,
               int32_t N, int32_t K, int32_t norm, int32_t relu, void* stream);

/* Split-fp16 image of a weight for nd_op_gemm_split (the engine's encoder
 * GEMMs): Wh [N][K/8][hi 8 | lo 8] fp16 halves of W * 2^s with hi = fp16(x),
 * lo = fp16(x - hi); *wscale receives 2^-s.  K % 32 == 0.  Synchronises the
 * stream (load-time operation). */
int nd_op_split_weight(const float* W, int32_t N, int32_t K, uint16_t* Wh, float* wscale, void* stream);

/* nd_op_gemm on a split weight: A is split the same way as it is staged and
 * the product summed as hi*hi + hi*lo + lo*hi on fp16 MFMAs with fp32
 * accumulation (22-bit operands; fp32-class results). */
int nd_op_gemm_split(const float* A, const uint16_t* Wh, float wscale, const float* bias, const float* R, float* C,
                     int32_t M, int32_t N, int32_t K, int32_t norm, int32_t relu, void* stream);

/* The decoder-step form of the same GEMM, on the fragment-packed "P16"
 * layout the engine keeps decoder activations and step weights in: an
 * [M, N] matrix (M, N multiples of 16) stored as 16x16 blocks in row-major
 * block order, each block 64 float4 entries, entry e = (m%16) + 16*((n%16)/4)
 * holding columns n&~3..+3 of row m (nd_op_pack_p16 converts).  A, W, R, C
 * packed.  LayerNorm prologue when part_in != NULL: per-row partial
 * statistics {mean_j, M2_j} of part_n_in equal column tiles at
 * part_in[(row*16 + j)*2]; part_out (nullable, N == 256) receives this
 * GEMM's output row partials, their count in *part_n_out. */
int nd_op_gemm_p16(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M,
                   int32_t N, int32_t K, const float* part_in, int32_t part_n_in, float* part_out, int32_t relu,
                   int32_t* part_n_out, void* stream);

/* Split-fp16 decoder-step GEMM: W as its P16H image (nd_op_pack_p16h:
 * [N/16][K/32][hi | lo][64 lanes][8 halves] of W * 2^s, *wscale = 2^-s from
 * a row-major W [N, K]; synchronises the stream), A split on the fly, the
 * product hi*hi + hi*lo + lo*hi on 16x16x32 f16 MFMAs into fp32.  Otherwise
 * exactly nd_op_gemm_p16. */
int nd_op_pack_p16h(const float* W, int32_t N, int32_t K, uint16_t* out, float* wscale, void* stream);
/* The encoder's fused position-wise FFN block (onmt/modules/position_ffn.py:
 * 27-40 as encoder/transformer.py:36-54 runs it): x = y + W2 relu(W1' LN(y)
 * + b1') + b2 over M rows of 256, y and x row-major [M, 256] (x != y), with
 * the LayerNorm affine folded into W1' / b1' (nd_op_fold_layernorm).  w1h /
 * w2h: P16H images (nd_op_pack_p16h) of W1' [F, 256] and W2 [256, F] with
 * their scales; F % 32 == 0, F <= 2048.  xpart (nullable) gets each row's
 * {mean, M2} at xpart[row * 32]; overflow (nullable) is set to 1 when a
 * hidden value leaves the fp16 range. */
int nd_op_enc_ffn(const float* y, const uint16_t* w1h, float w1s, const float* b1, const uint16_t* w2h, float w2s,
                  const float* b2, float* x, float* xpart, int32_t M, int32_t F, int32_t* overflow, void* stream);
/* The same block over the beam's decoder rows (decoder/transformer.py:92,
 * position_ffn.py:27-40): y and x P16-packed [M, 256] (M % 16 == 0, x != y),
 * the d_ff walk split over nsplit workgroups per 128-row block whose partial
 * sums meet in slab (nd_op_dec_ffn_slab_floats(M, nsplit) floats) and are
 * added in split order by the block's last workgroup (tickets: one int per
 * row block, zero before the launch and zero again after it).  skip
 * (nullable): per chunk of skip_rpc rows, nonzero = finished; a row block of
 * finished chunks is left as it was.  xpart: each row's {mean, M2} in one
 * partial.  Replaces the FFN1 + FFN2 GEMM pair of nd_translate_beam*'s step. */
int nd_op_dec_ffn(const float* y, const uint16_t* w1h, float w1s, const float* b1, const uint16_t* w2h, float w2s,
                  const float* b2, float* x, float* xpart, int32_t M, int32_t F, int32_t nsplit, float* slab,
                  int32_t* tickets, const int32_t* skip, int32_t skip_rpc, int32_t* overflow, void* stream);
int64_t nd_op_dec_ffn_slab_floats(int32_t M, int32_t nsplit);
/* The same block with the attention's output projection folded in front
 * (encoder/transformer.py:45-54, one launch for the rest of the layer):
 * y = x_in + att Wo^T + bo, then x = y + W2 relu(W1' LN(y) + b1') + b2.
 * woh: P16H image of Wo [256, 256] with its scale wos.  x may alias x_in
 * (the engine updates the layer's rows in place); att must not.  With qkvh
 * (nullable) the next layer's projection follows in the same launch:
 * qkv = LN(x) Wq'^T + qkvb (row-major [M, 768]; qkvh the P16H image of the
 * LN-folded Wq' [768, 256], qkvs its scale). */
int nd_op_enc_ffn_wo(const float* att, const float* x_in, const uint16_t* woh, float wos, const float* bo,
                     const uint16_t* w1h, float w1s, const float* b1, const uint16_t* w2h, float w2s, const float* b2,
                     float* x, float* xpart, const uint16_t* qkvh, float qkvs, const float* qkvb, float* qkv,
                     int32_t M, int32_t F, int32_t* overflow, void* stream);

int nd_op_gemm_p16_split(const float* A, const uint16_t* Wh, float wscale, const float* bias, const float* R, float* C,
                         int32_t M, int32_t N, int32_t K, const float* part_in, int32_t part_n_in, float* part_out,
                         int32_t relu, int32_t* part_n_out, void* stream);
/* The split-K form of the long-K decoder products (gemm_p16k_kernel: 32 x 32
 * tiles, K / 512 slices over workgroups, the slices summed in slice order by
 * the last arriving workgroup; the engine's route for W_vo and FFN2 at
 * 128 < rows <= 1024; decoder/transformer.py:88-93, position_ffn.py:38-40):
 * operands as nd_op_gemm_p16_split (no LN, no relu).  slab: >= tiles * 4096
 * floats; tickets: >= tiles int32, zero before the first call (each tile's
 * last arriver resets its own); tiles >= ceil(M / 32) * N / 32.  Fails if the
 * route is not taken. */
int nd_op_gemm_p16_splitk(const float* A, const uint16_t* Wh, float wscale, const float* bias, const float* R,
                          float* C, int32_t M, int32_t N, int32_t K, float* part_out, float* slab, int32_t* tickets,
                          int32_t tiles, int32_t* part_n_out, void* stream);

/* The same split-K route in exact fp32 (nd_set_exact_fp32: the pool lanes'
 * form of W_vo / FFN2 there): W is the fp32 weight [N, K] in the P16 layout
 * (as A), products on v_mfma_f32_16x16x4f32, no weight scale. */
int nd_op_gemm_p16_splitk_f32(const float* A, const float* W, const float* bias, const float* R, float* C,
                              int32_t M, int32_t N, int32_t K, float* part_out, float* slab, int32_t* tickets,
                              int32_t tiles, int32_t* part_n_out, void* stream);

/* The same GEMM with the weight's row-major split image too (nd_op_split_weight
 * of the row-major W): from M >= 2048 rows (beam search over large batches)
 * the engine runs it on the LDS-tiled kernel with P16 operands. */
int nd_op_gemm_p16_split_rm(const float* A, const uint16_t* Wh, float wscale, const uint16_t* Wh_rm, float wscale_rm,
                            const float* bias, const float* R, float* C, int32_t M, int32_t N, int32_t K,
                            const float* part_in, int32_t part_n_in, float* part_out, int32_t relu,
                            int32_t* part_n_out, void* stream);

/* row-major [M, N] -> P16 packed (M, N multiples of 16). */
int nd_op_pack_p16(const float* src, float* dst, int32_t M, int32_t N, void* stream);

/* Fold a LayerNorm's affine into the Linear that consumes it:
 * W_out = W diag(ln_g), b_out = bias + W ln_b (bias may be NULL), so that
 * Linear(LayerNorm(x)) == nd_op_gemm(x, W_out, b_out, norm = 1).  W [N,K]. */
int nd_op_fold_layernorm(const float* W, const float* bias, const float* ln_g, const float* ln_b, float* W_out,
                         float* b_out, int32_t N, int32_t K, void* stream);

/* Encoder self-attention over qkv [B*T, 3*d] (q | k | v) with the key mask
 * signal == 0.0 and keys >= span excluded; out [B*T, d]. */
int nd_op_enc_attention(const float* qkv, const float* signal, const int32_t* span, float* out, int32_t B,
                        int32_t T, void* stream);

/* The same with both of the engine's forms in reach: exact != 0 runs the fp32
 * kernel of nd_set_exact_fp32, exact == 0 the split-fp16 one, which sets
 * *overflow (nullable device int32, never cleared here) to 1 when a live K or
 * V element, or a live query element times log2(e) / sqrt(32), reaches 65504
 * in magnitude; the fp32 kernel never writes the word.  Rows t < span of out
 * are written, the others untouched; 1 <= span[b] (rows at or past span are
 * not read for their values and may hold anything).  A null qkv, signal, span
 * or out, or B < 1: ND_ERR_ARG before any HIP call; T outside 1..512:
 * ND_ERR_ARG, nothing launched. */
int nd_op_enc_attention_ex(const float* qkv, const float* signal, const int32_t* span, float* out, int32_t B,
                           int32_t T, int32_t exact, int32_t* overflow, void* stream);

/* Transformer encoder layer 0 up to (not including) W_o, as the engine runs
 * it: in closed form from the scalar samples (no x, no q | k | v rows), after
 * the same load-time preparation nd_finalize makes.  signal [B,T], span [B],
 * w_in / b_in [256] (the Linear(1, d) embedding), nwqkv [768,256] / nbqkv [768]
 * the layer's QKV with its LayerNorm affine folded (nd_op_fold_layernorm);
 * out [B*T,256]: rows t < min(span, T) written, the others untouched.  Key
 * mask signal == 0.0, keys >= span excluded.  Nullable device outputs of the
 * preparation: ac_out [6*256] floats (a [768], then c [768]), scal_out [4]
 * doubles (the means of w'^2, w' b_perp, b_perp^2, then s0: 0 while
 * cos^2(w', b') <= 1/16, else -mean(w' b') / mean(w'^2) in fp32), coef_out [48]
 * floats.  T outside 1..512, B < 1 or a null input: ND_ERR_ARG, nothing
 * launched.  Synchronises the stream. */
int nd_op_enc_layer0(const float* signal, const int32_t* span, const float* w_in, const float* b_in,
                     const float* nwqkv, const float* nbqkv, float* out, int32_t B, int32_t T, float* ac_out,
                     double* scal_out, float* coef_out, void* stream);

/* Decoder self-attention for one step (multi_headed_attn.py:124-141):
 * qkv [R, 3*d] and out [R, d] P16-packed (R padded to a multiple of 16);
 * cache [R, max_steps, 2*d] row-major (this step's k|v is appended at
 * [r][step]); anc nullable [R, anc_ld] slot ancestry (NULL = identity). */
int nd_op_dec_self_attention(const float* qkv, float* cache, const int32_t* anc, int32_t anc_ld, int32_t step,
                             int32_t max_steps, float* out, int32_t R, void* stream);
/* The same for beam rows, rpc (2..6) consecutive rows per chunk (R a
 * multiple of rpc) on the chunk-per-workgroup kernel the engine runs for
 * them: anc [R, anc_ld] required (each row's slots), done nullable [R / rpc]
 * (rows of chunks with done != 0 untouched, translate/translator.py:793-823). */
int nd_op_dec_self_attention_beam(const float* qkv, float* cache, const int32_t* anc, int32_t anc_ld, int32_t step,
                                  int32_t max_steps, float* out, int32_t R, int32_t rpc, const int32_t* done,
                                  void* stream);
/* The engine's form for beam rows outside exact fp32 (greedy rows keep the fp32 history above): the
 * cache holds each (slot, t) as 1600 bytes, k's 256 values as 24-bit
 * integers | v's | per head {k scale, v scale} (the layout of
 * nd_op_ctx_pack_q24's rows), [R, max_steps, 1600] bytes; this step's k|v
 * is quantised and appended.  rpc 1: the per-row kernel (anc nullable), 2..6:
 * the chunk kernel (anc required). */
int nd_op_dec_self_attention_q24(const float* qkv, void* cache, const int32_t* anc, int32_t anc_ld, int32_t step,
                                 int32_t max_steps, float* out, int32_t R, int32_t rpc, const int32_t* done,
                                 void* stream);
/* The greedy rows' layer-0 form (one row per chunk, no ancestry): table
 * [table_steps * V, 3*d] row-major holds q | k | v of input token v at step s
 * in row s * V + v.  Row r's own q | k | v is row step * V + tok[r] (step 0:
 * tok0 for every row, tok unused), its key t < step the k | v part of row
 * t * V + (t == 0 ? tok0 : hist[r * hist_ld + t - 1]): hist [R, hist_ld]
 * holds the token each row picked at every earlier step (values in [0, V)).
 * cache (nullable) is neither read nor written; out [R, d] P16-packed.
 * step < min(table_steps, max_steps). */
int nd_op_dec_self_attention_table(const float* table, int32_t table_steps, int32_t V, const int32_t* tok,
                                   int32_t tok0, const int32_t* hist, int32_t hist_ld, float* cache, int32_t step,
                                   int32_t max_steps, float* out, int32_t R, void* stream);

/* Memory-bank context attention (greedy form, model.hip
 * derive_memory_bank_weights; replaces the context MultiHeadedAttention of
 * decoder/transformer.py:88-92 for one row per chunk, rpc == 1): row c of
 * qp = Q' [C, 8*256] (P16; column block h = head h's query mapped into
 * memory space) attends over the row-major memory bank mem (chunk c's
 * position t at row c*ldT + t, T <= ldT) with keys t < span[c] and key mask
 * signal[c*T+t] == pad_val; out = U [C, 8*256] P16 (head h: the
 * softmax-weighted sum of memory rows).  grid > 0: that many workgroups walk
 * the chunks (the form nd_set_bank_grid selects for pool lanes). */
int nd_op_dec_mem_attention(const float* qp, const float* mem, const float* signal, const int32_t* span, float pad_val,
                            float* out, int32_t C, int32_t rpc, int32_t T, int32_t ldT, int32_t grid, void* stream);

/* One NanoEncoder BiLSTM layer, both directions (encoder/nano_encoder.py:92-111,
 * nn.LSTM(in, 128, bidirectional) over packed sequences): out [B*T, 256]
 * (fwd | bwd per row b*T + t) for t < len[b]; every value of a row t >= len[b]
 * is left as the caller set it or rewritten with exactly 0 (zero out before
 * the call for pad_packed_sequence's zeros).  layer0 != 0: input_size
 * 1, xp unused, the projection signal[b*T+t] * wih0[dir][g] + bsum[dir][g]
 * ([2][512] each) is formed in-kernel; otherwise xp [B*T, 1024] holds
 * x W_ih^T + b_ih + b_hh (fwd | bwd).  whh [2][512][128] (gates i, f, g, o).
 * bn_scale/bn_shift ([2][128], nullable): eval BatchNorm applied to the
 * written h. */
int nd_op_lstm_layer(const float* xp, const float* signal, const float* wih0, const float* bsum, const float* whh,
                     const int32_t* len, int32_t B, int32_t T, float* out, const float* bn_scale,
                     const float* bn_shift, int32_t layer0, void* stream);
/* The same layer in the exact-fp32 form (what nd_set_exact_fp32 selects in
 * the engine): fp32 MFMAs, 16 sequences per workgroup, libm activations.
 * Same arguments and refusals. */
int nd_op_lstm_layer_f32(const float* xp, const float* signal, const float* wih0, const float* bsum, const float* whh,
                         const int32_t* len, int32_t B, int32_t T, float* out, const float* bn_scale,
                         const float* bn_shift, int32_t layer0, void* stream);

/* Encoder output x [B*T, 256] row-major -> memory bank, row-major with ldT
 * rows per chunk (LayerNorm with ln_g/ln_b when ln_g != NULL,
 * encoder/transformer.py:125; rows t >= T zero). */
int nd_op_memory_pack(const float* x, const float* ln_g, const float* ln_b, float* out, int32_t B, int32_t T,
                      int32_t ldT, void* stream);

/* 24-bit fixed-point memory bank (the greedy decoder's context attention at
 * every chunk length T <= 512; multi_headed_attn.py:142-177 in the memory-bank form of
 * nd_op_dec_mem_attention).  nd_op_bank_pack_d8: x [B*T, 256] row-major -> the
 * digit bank (B x 512 rows; every row t as s_t times an integer of at most
 * 126 * 2^16 in magnitude in three signed 8-bit digit planes, B * 512 * 256 *
 * 3 bytes in the v_mfma_i32_16x16x64_i8 A-operand fragment order), kscale
 * [B * 512] floats (s_t) and kemax [B] (each chunk's largest s_t, float bits);
 * LayerNorm with ln_g/ln_b when set; rows t >= T, and rows t >= span[c] when
 * span (nullable, [B]) is given, zero with scale 0 (the engine passes the
 * call's spans: rows past a chunk's span are never attended and must not set
 * its largest scale).  nd_op_dec_bank_d8: qp [C, 2048] ROW-MAJOR (one row
 * per chunk), T in [1, 512] (the first ceil(T / 128) key blocks of each wave
 * streamed); out U [C16, 2048] P16.  grid: workgroups at
 * most (0 = one per chunk; fewer walk the chunks, as nd_set_bank_grid).  ovf
 * (nullable): set to 1 on a non-finite operand. */
int nd_op_bank_pack_d8(const float* x, const float* ln_g, const float* ln_b, void* bank, float* kscale,
                       int32_t* kemax, const int32_t* span, int32_t B, int32_t T, int32_t* ovf, void* stream);
int nd_op_dec_bank_d8(const float* qp, const void* bank, const float* kscale, const int32_t* kemax,
                      const float* signal, const int32_t* span, float pad_val, float* out, int32_t C, int32_t T,
                      int32_t* ovf, int32_t grid, void* stream);

/* Which memory bank the context's last call streamed (diagnostics, the
 * bench's roofline accounting): 0 fp32 bank, or fp32 K/V (a beam call in
 * exact fp32), 2 24-bit digits (nd_op_dec_bank_d8), 3 the 24-bit context K/V
 * of a beam call (nd_op_dec_ctx_attention_q24).  (1, the split-fp16 bank of
 * rounds 2-3, is retired.) */
int nd_bank_form(nd_ctx* ctx);

/* Decoder context attention (multi_headed_attn.py:142-177): rows r = c*rpc+j
 * of q [C*rpc, d] attend over K at kv[(c*T+t)*ld + koff] and V at +d, keys
 * t < span[c], key mask signal == pad_val; out [C*rpc, d].  q and out are
 * P16-packed (rows padded to a multiple of 16), kv row-major. */
int nd_op_dec_ctx_attention(const float* q, const float* kv, int32_t ld, int32_t koff, const float* signal,
                            const int32_t* span, float pad_val, float* out, int32_t C, int32_t rpc, int32_t T,
                            void* stream);

/* The beam's context K/V in 24-bit fixed point (the default for beam rows
 * outside exact fp32; the same attention as nd_op_dec_ctx_attention,
 * multi_headed_attn.py:142-177, on 0.78x the bytes).  nd_op_ctx_pack_q24:
 * fp32 K/V kv [B*T, ld] (layer l's k at column l*512, v at l*512+256; the
 * reference's linear_keys / linear_values outputs, multi_headed_attn.py:
 * 142-150) -> image out [layers][B*T][1600 B] (layer-major: one layer's
 * keys of a chunk are contiguous): per (layer, key) k's 256
 * values as 24-bit integers (3 bytes each; the 12 bytes at 12*i hold dims
 * 4i..4i+3), v's at byte 768, then per head h {2^(e_k - 23), 2^(e_v - 23)}
 * as floats at byte 1536 + 8h, with e the head's exponent (max|x| < 2^e); an
 * element's error is at most 2^-23 of its head's largest |x|.  Rows t >=
 * span[c] are not written.  nd_op_dec_ctx_attention_q24: as
 * nd_op_dec_ctx_attention with K/V of layer `layer` from that image (C*T
 * rows per layer plane). */
int nd_op_ctx_pack_q24(const float* kv, int32_t ld, int32_t layers, void* out, const int32_t* span, int32_t B,
                       int32_t T, void* stream);
/* The engine's form: the memory's K / V projection (split-fp16, as
 * nd_op_gemm_split, N = layers * 512) whose epilogue writes that image
 * (layer planes of plane_rows >= M rows) instead of fp32 K / V; every row
 * is written. */
int nd_op_gemm_split_q24(const float* A, const uint16_t* Wh, float wscale, const float* bias, void* img,
                         int32_t plane_rows, int32_t M, int32_t N, int32_t K, int32_t norm, void* stream);
int nd_op_dec_ctx_attention_q24(const float* q, const void* kvq, int32_t layers, int32_t layer, const float* signal,
                                const int32_t* span, float pad_val, float* out, int32_t C, int32_t rpc, int32_t T,
                                void* stream);

/* The --fast beam tail's forms (translate/translator.py:793-823 drops
 * finished batches; the engine launches over the alive chunks only once at
 * most a sixteenth of them remain).  nd_op_alive_list: chunks c < C with
 * done[c] == 0, ascending, into list[0 .. cap), the rest -1; more than cap
 * alive sets *ovf (nullable) to 1.  nd_op_dec_ctx_attention_list: the context
 * attention (fp32 K/V, or one layer plane of the 24-bit image when q24 != 0,
 * ld = 1600 and koff = 0 bytes) for the listed chunks only (list entries -1 and chunks with done[c]
 * != 0 untouched), each chunk's keys in nsplit workgroups (1..64) whose
 * partial softmax states go to part (ccap * nsplit * rpc * 272 floats) and
 * are combined by a second launch. */
int nd_op_alive_list(const int32_t* done, int32_t C, int32_t* list, int32_t cap, int32_t* ovf, void* stream);
int nd_op_dec_ctx_attention_list(const float* q, const void* kv, int32_t ld, int32_t koff, int32_t q24,
                                 const float* signal, const int32_t* span, float pad_val, float* out, int32_t C,
                                 int32_t rpc, int32_t T, const int32_t* clist, int32_t ccap, int32_t nsplit,
                                 float* part, const int32_t* done, void* stream);

/* The scoring pass's attention (score.hip tf_attention_kernel), fp32, 8 heads of 32: Lq query rows per
 * chunk (row c * Lq + i of q, pitch ldq floats) over the chunk's Lk key rows (row c * Lk + t of kv, pitch
 * ldkv; K at column koff, V at column voff); out [B * Lq, 256] row-major.  causal != 0: keys j <= i
 * (Lq == Lk; signal and span unused, may be null).  causal == 0: keys t < span[c], those with
 * signal[c * Lk + t] == pad_val filled with -1e18 (multi_headed_attn.py:142-177), as
 * nd_op_dec_ctx_attention. */
int nd_op_tf_attention(const float* q, int32_t ldq, const float* kv, int32_t ldkv, int32_t koff, int32_t voff,
                       const float* signal, const int32_t* span, float pad_val, float* out, int32_t B, int32_t Lq,
                       int32_t Lk, int32_t causal, void* stream);
/* nd_op_tf_attention of the context attention (causal must be 0: ND_ERR_ARG otherwise) that also stores
 * head 0's scores after the mask and before the softmax: tap[(c * Lq + i) * ld_tap + t] for i < Lq and
 * t < min(span[c], Lk) (and up to the end of that key's block of 32, below Lk) = the fp32 score, -1e18 for
 * a masked key, -inf for a key at or past span[c].  ld_tap >= Lk floats (ND_ERR_ARG otherwise); columns at
 * or past Lk are never written.  16-byte stores when ld_tap and the buffer's address are multiples of 4
 * floats, scalar stores otherwise.  out is bit for bit nd_op_tf_attention's. */
int nd_op_tf_attention_tap(const float* q, int32_t ldq, const float* kv, int32_t ldkv, int32_t koff, int32_t voff,
                           const float* signal, const int32_t* span, float pad_val, float* out, int32_t B, int32_t Lq,
                           int32_t Lk, int32_t causal, float* tap, int32_t ld_tap, void* stream);

/* ---- output head and search, one launch per call ------------------------
 * The kernels that turn log-probs into output (search.hip, head.hpp), each on
 * the caller's stream with caller-owned buffers, for op-level tests against a
 * scripted model.  Decoder rows x and the next step's input ne_x are P16
 * [R16, 256] (R16 = rows rounded up to 16; nd_op_pack_p16); ne_part holds
 * R16 * 32 floats (each row's {mean, M2} at ne_part[row * 32]); ne_tok
 * (nullable) [rows] i32.  The head: ln_g / ln_b [256] (LayerNorm, eps 1e-6),
 * gw [V, 256] / gb [V] (generator), log_softmax; emb [V, 256], pe (nullable:
 * no position encoding and no sqrt(d) scale) [>= S, 256].  A null buffer, a
 * step outside [0, S), eos outside [0, V) or a count below 1 returns
 * ND_ERR_ARG "<entry>: bad arguments" before any HIP call; the launchers'
 * own refusals (named per entry below) follow, also before any launch. */

/* The search state of the beam kernels (kernels.hpp BeamState, member for
 * member; the classic Beam's members may be null for the --fast beam, cov /
 * pen / prev_pen / attn / cut without a coverage penalty, blk without n-gram
 * blocking).  C chunks of beam rows, row = c * beam + j. */
typedef struct nd_beam_state {
  float* cum;          /* [C, beam] */
  int32_t* seq[2];     /* [C*beam, S] double buffered: step s reads [s & 1], writes the other */
  int32_t* anc[2];     /* [C*beam, S] */
  int32_t* tok;        /* [C*beam] */
  int32_t* done;       /* [C] */
  int32_t* top_fin;    /* [C] */
  int32_t* n_hyp;      /* [C] */
  float* hyp_score;    /* [C, n_best] */
  int32_t* hyp_len;    /* [C, n_best] */
  int32_t* hyp_tok;    /* [C, n_best, S] */
  int32_t* n_alive;    /* [1] */
  int32_t* steps_done; /* [1] */
  int32_t* group;      /* [C] classic */
  int32_t* grp_left;   /* [C] classic */
  int32_t* grp_done;   /* [C] classic: 0 alive, else 1 + the step the batch finished in */
  int32_t* steps_run;  /* [C] */
  int32_t* hyp_anc;    /* [C, n_best, S] */
  float* cov[2];       /* [C*beam, T] */
  float* pen;          /* [C*beam] */
  float* prev_pen;     /* [C*beam] */
  int32_t* blk[2];     /* [C*beam] */
  const float* attn;   /* [C*beam, S, T] */
  const int32_t* cut;  /* [C] */
  int32_t T;
} nd_beam_state;

/* One greedy head launch over R rows for `step` (translate/translator.py:
 * 371-394, 455-483; models/model_builder.py:326-334): tok [R], out_tokens
 * [R, S] (column step written), score [R], logp (nullable) [R, S, V] (row
 * [r][step] written, before the min_len mask), and for step + 1 < S the next
 * input rows ne_x / ne_part / ne_tok (embeddings.py:189-207).  d_seed
 * (nullable, a device word): random sampling with temp and topk (-1: the
 * whole distribution) from the counter-based generator of nd_translate_sample.
 * Refused ("greedy_head: "): V outside [1, 32]; with d_seed, temp == 0,
 * topk == 1 or topk > V. */
int nd_op_greedy_head(const float* x, const float* ln_g, const float* ln_b, const float* gw, const float* gb, int32_t V,
                      int32_t S, int32_t step, int32_t min_len, int32_t eos, int32_t R, const float* emb,
                      const float* pe, float* ne_x, float* ne_part, int32_t* ne_tok, int32_t* tok,
                      int32_t* out_tokens, float* score, float* logp, float temp, int32_t topk,
                      const uint64_t* d_seed, void* stream);

/* The --fast beam (translate/translator.py:619-825), no reference equivalent
 * as separate calls: init (:691-693), one step (:701-823: head, length
 * penalty ((5 + step + 1) / 6) ** alpha as the engine computes it, top-beam,
 * reorder, finished-hypothesis bookkeeping, next input rows), finish (tokens
 * [C, n_best, S] -1 padded, scores and lens [C, n_best]).  clist (nullable):
 * the step runs the ccap listed chunks only (-1 = none).  Refused
 * ("beam_step: "): V outside [1, 32], beam outside [1, 8], beam * V > 256,
 * n_best outside [1, beam], ccap outside [1, C]. */
int nd_op_beam_init(const nd_beam_state* st, int32_t C, int32_t beam, int32_t bos, void* stream);
int nd_op_beam_step(const float* x, const float* ln_g, const float* ln_b, const float* gw, const float* gb, int32_t V,
                    const float* emb, const float* pe, float* ne_x, float* ne_part, int32_t* ne_tok,
                    const nd_beam_state* st, int32_t C, int32_t beam, int32_t n_best, int32_t step, int32_t S,
                    int32_t min_len, int32_t eos, float alpha, const int32_t* clist, int32_t ccap, void* stream);
int nd_op_beam_finish(const nd_beam_state* st, int32_t C, int32_t n_best, int32_t S, int32_t* tokens, float* scores,
                      int32_t* lens, void* stream);

/* The classic onmt Beam (translate/translator.py:827-926, onmt/translate/
 * beam.py:6-243): init (group [C]: each chunk's reference batch), one step
 * (Beam.advance for every chunk of a batch still alive, st->attn / cut / T
 * read by the coverage penalties), finish (sort_finished(minimum = n_best)).
 * Refused ("beam_classic_step: "): as beam_step, and V < beam, a coverage
 * penalty without st->attn / cut / cov, n-gram blocking without st->blk;
 * ("beam_classic_finish: ") n_best > beam. */
int nd_op_beam_classic_init(const nd_beam_state* st, const int32_t* group, int32_t C, int32_t beam, int32_t bos,
                            void* stream);
int nd_op_beam_classic_step(const float* x, const float* ln_g, const float* ln_b, const float* gw, const float* gb,
                            int32_t V, const float* emb, const float* pe, float* ne_x, float* ne_part,
                            int32_t* ne_tok, const nd_beam_state* st, int32_t C, int32_t beam, int32_t n_best,
                            int32_t step, int32_t S, int32_t min_len, int32_t eos, const nd_classic_opts* opts,
                            void* stream);
int nd_op_beam_classic_finish(const nd_beam_state* st, int32_t C, int32_t beam, int32_t n_best, int32_t S,
                              const nd_classic_opts* opts, int32_t* tokens, float* scores, int32_t* lens,
                              void* stream);

/* -attn_debug / coverage capture.  nd_op_attn_step_softmax: in place, row r
 * of R (chunk r / rpc) at a[r * ld + t]: softmax over keys t < min(span[chunk],
 * T), zero for the other t < T (multi_headed_attn.py:175).
 * nd_op_beam_attn_gather: out [C, n_best, max_len, T], row t of hypothesis k =
 * st->attn[hyp_anc[c][k][t]][t][0 .. T) for t < hyp_len[c][k], zero after
 * (translate/translator.py:745-751); refused when st->attn is null,
 * T > st->T or max_len > S. */
int nd_op_attn_step_softmax(float* a, int64_t ld, const int32_t* span, int32_t R, int32_t rpc, int32_t T,
                            void* stream);
int nd_op_beam_attn_gather(const nd_beam_state* st, int32_t C, int32_t n_best, int32_t S, int32_t max_len, int32_t T,
                           float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NANODEC_H */
