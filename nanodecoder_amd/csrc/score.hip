// Teacher-forced scoring (translate/translator.py:928-941, Translator._score_target): the decoder over a
// whole target in one pass.  All L positions of all B chunks are B * L independent, row-major decoder rows;
// the GEMMs are the encoder's (gemm.hip).  This file holds what those do not cover:
//
// * tf_embed_kernel: row (c, i) = the embedding of BOS (i == 0) or of the gold token i - 1, with its
//   LayerNorm statistics for the QKV GEMM's prologue.
// * tf_attention_kernel<CAUSAL>: flash-style fp32 attention whose query rows are not its key rows: the
//   decoder self-attention over the target (causal, keys j <= i) and the context attention over the chunk's
//   memory keys (span and pad mask).  Modelled on enc_attention_kernel (attention.hip): scores transposed
//   (S^T = K Q^T on v_mfma_f32_32x32x2_f32) so a lane holds one query's 32 scores, online softmax and O in
//   registers, one wave per 32 query rows.  K / V^T stream through LDS in tiles of TF_KT keys (35,840 B
//   static: K 18,432 at stride 36, V^T 16,896 at stride 132, flags 512), the next tile's global loads in
//   flight under the current tile's arithmetic.  tf_attention_kernel<false, true> is the same kernel that
//   also stores its head-0 scores (the tap of nd_score_targets_attn).
// * score_head_kernel: final LayerNorm, generator, log-softmax, the gold token's log-probability per row,
//   and their sum per chunk in a fixed order (no float atomics).
// * cand_posterior_kernel: K candidate targets per chunk (nd_score_candidates): the log-posterior over a
//   chunk's candidates and the best of them from their K scores.
#include "common.hpp"
#include "kernels.hpp"

namespace nd {

#define TF_NW 4      // waves per workgroup = query blocks of 32 rows
#define TF_KT 128    // keys per LDS tile (= TF_NW * 32: a workgroup's causal diagonal is one tile)
#define TF_KLD 36    // K row stride (floats): conflict-free ds_read_b128
#define TF_VLD 132   // V^T row stride
#define TF_MAXL 512  // target positions at most (nd_create: max_steps <= 512)

__device__ __forceinline__ void tf_row_part(f32x4 v, int lane, float* part) {
  const float mu = wave_sum(v.x + v.y + v.z + v.w) * (1.0f / ND_D);
  const f32x4 d = v - mu;
  const float q = wave_sum(d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w);
  if (lane == 0) {
    part[0] = mu;
    part[1] = q;
  }
}

// onmt/modules/embeddings.py:189-207 (+ PositionalEncoding.forward :36-43) for every target position at
// once: the arithmetic of dec_embed_kernel (attention.hip) at step i, row-major
__global__ void __launch_bounds__(256)
tf_embed_kernel(const int* __restrict__ gold, int bos, int V, const float* __restrict__ emb,
                const float* __restrict__ pe, float* __restrict__ x, float* __restrict__ part, int rows, int L) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int c = row / L, i = row - c * L;
  const int g = gold[(size_t)c * L + max(i - 1, 0)];
  const int tk = min(max(i == 0 ? bos : g, 0), V - 1);  // a bad id never indexes out of the table
  f32x4 e = ld4(emb + (size_t)tk * ND_D + lane * 4);
  if (pe) e = e * 16.0f + ld4(pe + (size_t)i * ND_D + lane * 4);  // sqrt(256) = 16
  st4(x + (size_t)row * ND_D + lane * 4, e);
  tf_row_part(e, lane, part + (size_t)row * ND_PART_LD * 2);
}

hipError_t launch_tf_embed(const int* gold, int bos, int V, const float* emb, const float* pe, float* x, float* part,
                           int B, int L, hipStream_t s) {
  if (B < 1 || L < 1 || V < 1) return hipErrorInvalidValue;
  const int rows = B * L;
  hipLaunchKernelGGL(tf_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, gold, bos, V, emb, pe, x, part, rows, L);
  return hipGetLastError();
}

// Workgroup (head h, query group g, chunk c): waves 0..3 own query rows 128 g + 32 w .. + 31 of the chunk.
// Rows at or past Lq are clamped to the last row (computed, never stored); keys at or past the chunk's key
// count are clamped loads flagged absent.  Every load is unconditional ("Straight-line
// loads").
// TAP (context attention only): the head-0 workgroups also store every score they walk, after the mask and
// before the online softmax, at tap[(c * Lq + qi) * ld_tap + t] for the rows qi < Lq and the keys t < Lk
// (forced alignment).  In the transposed layout a lane's register group r = 4g .. 4g+3
// is four consecutive keys of its query, so a group is one 16-byte store where the rows allow it (ld_tap and
// the buffer's address multiples of 4 floats) and four scalar stores otherwise; lanes l and l + 32 together
// write a row's 32 keys of the block, one whole 128-byte segment.  O, m and l do not know the tap exists.
template <bool CAUSAL, bool TAP = false>
__global__ void __launch_bounds__(TF_NW * 64)
tf_attention_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kv, int ldkv, int koff, int voff,
                    const float* __restrict__ signal, const int* __restrict__ span, float pad_val,
                    float* __restrict__ out, int Lq, int Lk, float* __restrict__ tap, int ld_tap) {
  static_assert(!(CAUSAL && TAP), "the tap is the context attention's");
  __shared__ __attribute__((aligned(16))) float Ks[TF_KT * TF_KLD];
  __shared__ __attribute__((aligned(16))) float Vt[ND_DH * TF_VLD];
  __shared__ int kflag[TF_KT];  // 0 = key, 1 = masked (signal == pad_val), 2 = absent (t >= span)

  const int h = blockIdx.x, qg = blockIdx.y, c = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  // keys of the chunk; a causal workgroup walks the tiles up to its diagonal one only
  const int nk = CAUSAL ? Lk : max(1, min(span[c], Lk));
  const int klim = CAUSAL ? min(nk, (qg + 1) * TF_KT) : nk;
  const int ntile = (klim + TF_KT - 1) / TF_KT;
  const size_t kbase = (size_t)c * Lk;

  // staging: thread items p = 0..3 are (key tid / 8 + 32 p, dims 4 (tid % 8) .. + 3) of the tile
  const int sk = tid >> 3, sc = (tid & 7) * 4;
  f32x4 kr[4], vr[4];
  float sr[4];
  auto gload = [&](int tile) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int t = min(tile * TF_KT + sk + 32 * p, nk - 1);
      const float* row = kv + (kbase + t) * (size_t)ldkv + h * ND_DH + sc;
      kr[p] = ld4(row + koff);
      vr[p] = ld4(row + voff);
      if constexpr (!CAUSAL) sr[p] = signal[kbase + t];
    }
  };
  auto sstore = [&](int tile) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int tl = sk + 32 * p;
      st4(&Ks[tl * TF_KLD + sc], kr[p]);
      Vt[(sc + 0) * TF_VLD + tl] = vr[p].x;
      Vt[(sc + 1) * TF_VLD + tl] = vr[p].y;
      Vt[(sc + 2) * TF_VLD + tl] = vr[p].z;
      Vt[(sc + 3) * TF_VLD + tl] = vr[p].w;
      if constexpr (!CAUSAL) {
        if (sc == 0) kflag[tl] = tile * TF_KT + tl < nk ? (sr[p] == pad_val ? 1 : 0) : 2;
      }
    }
  };

  const int q0 = (qg * TF_NW + wave) * 32;
  const int qi = q0 + lr;
  const bool active = q0 < Lq;  // wave-uniform; idle waves still stage and meet the barriers
  // TAP: every tapped row starts on a 16-byte boundary (workgroup-uniform)
  const bool tap_v4 = TAP && (ld_tap & 3) == 0 && (reinterpret_cast<uintptr_t>(tap) & 15) == 0;
  // query fragment: step s = 4j+i uses d = 8j + 4*lh + i; pre-scaled like
  // ``query / math.sqrt(dim_per_head)`` (multi_headed_attn.py:167)
  f32x4 qf[4];
  {
    const float* qrow = q + ((size_t)c * Lq + min(qi, Lq - 1)) * (size_t)ldq + h * ND_DH + 4 * lh;
#pragma unroll
    for (int j = 0; j < 4; ++j) qf[j] = ld4(qrow + 8 * j) / ND_SQRT_DH;
  }
  gload(0);

  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int tile = 0; tile < ntile; ++tile) {
    sstore(tile);
    lds_barrier();
    gload(min(tile + 1, ntile - 1));  // lands under this tile's arithmetic
    if (active) {
      // 32-key blocks of the tile this wave needs: up to the chunk's keys, causal: up to its diagonal block
      const int kend = CAUSAL ? min(nk, q0 + 32) : nk;
      const int ns = min(TF_KT / 32, (kend - tile * TF_KT + 31) / 32);
      for (int s = 0; s < ns; ++s) {
        const int key0 = tile * TF_KT + s * 32;
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
        const float* krow = &Ks[(s * 32 + lr) * TF_KLD + 4 * lh];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 kf = ld4(krow + 8 * j);
#pragma unroll
          for (int i = 0; i < 4; ++i) sacc = mfma32(kf[i], qf[j][i], sacc);
        }
        // sacc[r] = score(query qi, key key0 + mfma32_row(r, lane))
        float mx = -INFINITY;
        if constexpr (CAUSAL) {
          if (key0 == q0) {  // the diagonal tile: keys j <= i
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = mfma32_row(r, lane) > lr ? -INFINITY : sacc[r];
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int f = kflag[s * 32 + mfma32_row(r, lane)];
            float sv = sacc[r];
            sv = f == 1 ? ND_MASK_FILL : sv;
            sv = f == 2 ? -INFINITY : sv;
            sacc[r] = sv;
            mx = fmaxf(mx, sv);
          }
          if constexpr (TAP) {
            if (h == 0 && qi < Lq) {
              const int t0 = key0 + 4 * lh;  // group g holds keys t0 + 8g .. + 3
              float* trow = tap + ((size_t)c * Lq + qi) * (size_t)ld_tap + t0;
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                if (tap_v4 && t0 + 8 * g + 4 <= Lk) {
                  const f32x4 v = {sacc[4 * g + 0], sacc[4 * g + 1], sacc[4 * g + 2], sacc[4 * g + 3]};
                  st4(trow + 8 * g, v);
                } else {
#pragma unroll
                  for (int i = 0; i < 4; ++i)
                    if (t0 + 8 * g + i < Lk) trow[8 * g + i] = sacc[4 * g + i];
                }
              }
            }
          }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = __expf(m - mn);
        float rsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sacc[r] = __expf(sacc[r] - mn);
          rsum += sacc[r];
        }
        rsum += __shfl_xor(rsum, 32, 64);
        l = l * alpha + rsum;
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
        // O^T[d][q] += V^T[d][key] P^T[key][q]; step s = 4j+i uses key 8j + 4*lh + i
        const float* vrow = &Vt[lr * TF_VLD + s * 32 + 4 * lh];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 vf = ld4(vrow + 8 * j);
#pragma unroll
          for (int i = 0; i < 4; ++i) o = mfma32(vf[i], sacc[4 * j + i], o);
        }
      }
    }
    // every wave is done with the tile before the next one overwrites it.  The s_nop: the epilogue reads O
    // right behind the loop, and hipcc left 17 wait states between the last 32x32x2 MFMA and that read on the
    // path through this barrier where tools/isa_hazard.py asks for 18
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier\n\ts_nop 3" ::: "memory");
  }
  if (active && qi < Lq) {
    const float inv = 1.0f / l;
    float* orow = out + ((size_t)c * Lq + qi) * ND_D + h * ND_DH + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v = {o[4 * g + 0] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
      st4(orow + 8 * g, v);
    }
  }
}

hipError_t launch_tf_attention(const TfAttnArgs& a, hipStream_t s) {
  const SrcMask& m = a.mask;
  if (!a.q || !a.kv || !a.out || a.B < 1 || a.B > 65535 || a.Lq < 1 || a.Lk < 1) return hipErrorInvalidValue;
  if (a.ldq < ND_D || a.ldkv < ND_D || (a.ldq | a.ldkv | a.koff | a.voff) % 4 || a.koff < 0 || a.voff < 0 ||
      a.koff + ND_D > a.ldkv || a.voff + ND_D > a.ldkv)
    return hipErrorInvalidValue;
  if (a.causal ? a.Lq != a.Lk : (!m.signal || !m.span)) return hipErrorInvalidValue;
  if (a.tap && (a.causal || a.ld_tap < a.Lk)) return hipErrorInvalidValue;  // the tap: context attention only
  const dim3 grid(ND_H, (a.Lq + TF_NW * 32 - 1) / (TF_NW * 32), a.B), block(TF_NW * 64);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, block, 0, s, a.q, a.ldq, a.kv, a.ldkv, a.koff, a.voff, m.signal, m.span, m.pad_val,
                       a.out, a.Lq, a.Lk, a.tap, a.ld_tap);
  };
  if (a.causal)
    go(tf_attention_kernel<true>);
  else if (a.tap)
    go(tf_attention_kernel<false, true>);
  else
    go(tf_attention_kernel<false>);
  return hipGetLastError();
}

// LN + generator + log_softmax of one row-major row, held by one wave: head_row (head.hpp) with the row
// read row-major, same arithmetic in the same order.  Writes logp[0..V) to lp (LDS; every lane writes the
// same values).
__device__ __forceinline__ void tf_head_row(const float* __restrict__ xrow, const float* __restrict__ ln_g,
                                            const float* __restrict__ ln_b, const float* __restrict__ gw,
                                            const float* __restrict__ gb, int V, int lane, float* lp) {
  f32x4 wr[8];
  float br[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    wr[k] = ld4(gw + (size_t)min(k, V - 1) * ND_D + lane * 4);
    br[k] = gb[min(k, V - 1)];
  }
  f32x4 v = ld4(xrow + lane * 4);
  const f32x4 g = ld4(ln_g + lane * 4), bt = ld4(ln_b + lane * 4);
  const float mu = wave_sum(v.x + v.y + v.z + v.w) * (1.0f / ND_D);
  const f32x4 d = v - mu;
  const float var = wave_sum(d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w) * (1.0f / ND_D);
  const float rs = ln_rsqrt(var + ND_LN_EPS);
  const f32x4 y = d * rs * g + bt;
  float mx = -INFINITY;
  for (int k0 = 0; k0 < V; k0 += 8) {
    if (k0 > 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        wr[k] = ld4(gw + (size_t)min(k0 + k, V - 1) * ND_D + lane * 4);
        br[k] = gb[min(k0 + k, V - 1)];
      }
    }
    float dt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) dt[k] = y.x * wr[k].x + y.y * wr[k].y + y.z * wr[k].z + y.w * wr[k].w;
#pragma unroll
    for (int k = 0; k < 8; ++k) dt[k] = wave_sum(dt[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k0 + k < V) {
        const float logit = dt[k] + br[k];
        lp[k0 + k] = logit;
        mx = fmaxf(mx, logit);
      }
  }
  // torch log_softmax: (x - max) - log(sum(exp(x - max)))
  float s = 0.f;
  for (int k = 0; k < V; ++k) s += expf(lp[k] - mx);
  const float ls = logf(s);
  for (int k = 0; k < V; ++k) lp[k] = (lp[k] - mx) - ls;
}

#define TF_HW 8  // waves of the scoring head's workgroup

// One workgroup per chunk: its waves walk the chunk's rows (row i on wave i % 8), each row's gold
// log-probability goes to LDS, and wave 0 sums them in an order that depends on nothing but the position
// (lane i % 64 adds positions i, i + 64, ... in turn, then the wave's butterfly): the same bits whatever L
// the chunk is padded to.  _score_target zeroes the pad column and sums over every position: positions at or
// past gold_len add exactly 0.
__global__ void __launch_bounds__(TF_HW * 64)
score_head_kernel(const float* __restrict__ x, const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                  const float* __restrict__ gw, const float* __restrict__ gb, int V, const int* __restrict__ gold,
                  const int* __restrict__ gold_len, int L, float* __restrict__ score, float* __restrict__ tok_logp,
                  float* __restrict__ logp) {
  __shared__ float lps[TF_MAXL];
  __shared__ float lpw[TF_HW][ND_MAXV];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(gold_len[c], 0), L);
  for (int i = wave; i < L; i += TF_HW) {
    const size_t row = (size_t)c * L + i;
    const int g = min(max(gold[row], 0), V - 1);
    float* lp = lpw[wave];
    tf_head_row(x + row * ND_D, ln_g, ln_b, gw, gb, V, lane, lp);
    const float v = i < n ? lp[g] : 0.f;
    if (logp && lane < V) logp[row * V + lane] = lp[lane];
    if (lane == 0) {
      lps[i] = v;
      if (tok_logp) tok_logp[row] = v;
    }
  }
  __syncthreads();
  if (wave == 0) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < TF_MAXL / 64; ++k) {
      const int i = lane + 64 * k;
      acc += i < n ? lps[i] : 0.f;
    }
    acc = wave_sum(acc);
    if (lane == 0) score[c] = acc;
  }
}

hipError_t launch_score_head(const Generator& g, const int* gold, const int* gold_len, int B, int L, float* score,
                             float* tok_logp, float* logp, hipStream_t s) {
  if (B < 1 || L < 1 || L > TF_MAXL || g.V < 1 || g.V > ND_MAXV || !score) return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_head_kernel, dim3(B), dim3(TF_HW * 64), 0, s, g.x, g.ln_g, g.ln_b, g.gw, g.gb, g.V, gold,
                     gold_len, L, score, tok_logp, logp);
  return hipGetLastError();
}

// Candidate posterior (nd_score_candidates, nd_cand_posterior): one chunk per thread,
// its K slots walked in slot order three times (maximum and best, sum, outputs), so a chunk's bits depend on
// nothing but its own K scores.  A slot is empty when its cand_len <= 0: it reads -inf in score_out and post
// and takes no part.  m = the maximum over the other slots (updated by s > m: the lowest slot wins a tie, a
// NaN is never best), sum = the sum of expf(s_k - m) in slot order, post_k = (s_k - m) - logf(sum): a NaN
// score makes every post of its chunk NaN.  Each slot's score is read before score_out[slot] is written, so
// score_out may be score (no __restrict__ on the two).
__global__ void __launch_bounds__(256)
cand_posterior_kernel(const float* score, const int* __restrict__ cand_len, int B, int K, float* score_out,
                      float* __restrict__ post, int* __restrict__ best) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= B) return;
  const float* sc = score + (size_t)c * K;
  const int* cl = cand_len + (size_t)c * K;
  float m = -INFINITY;
  int bk = -1;
  for (int k = 0; k < K; ++k) {
    if (cl[k] <= 0) continue;
    const float s = sc[k];
    if (s > m || (bk < 0 && s == m)) {  // s == m with no best yet: a score of -inf itself
      m = s;
      bk = k;
    }
  }
  float sum = 0.f;
  for (int k = 0; k < K; ++k)
    if (cl[k] > 0) sum += expf(sc[k] - m);
  const float ls = logf(sum);
  for (int k = 0; k < K; ++k) {
    const bool live = cl[k] > 0;
    const float s = sc[k];
    score_out[(size_t)c * K + k] = live ? s : -INFINITY;
    if (post) post[(size_t)c * K + k] = live ? (s - m) - ls : -INFINITY;
  }
  if (best) best[c] = bk;
}

hipError_t launch_cand_posterior(const float* score, const int* cand_len, int B, int K, float* score_out, float* post,
                                 int* best, hipStream_t s) {
  if (!score || !cand_len || !score_out || B < 1 || K < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cand_posterior_kernel, dim3((B + 255) / 256), dim3(256), 0, s, score, cand_len, B, K, score_out,
                     post, best);
  return hipGetLastError();
}

}  // namespace nd
