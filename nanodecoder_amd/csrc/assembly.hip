// Read assembly on the device: the overlap consensus of
// utils/labelop.py:310-352 (simple_assembly / add_count) for a whole group of
// reads, byte-identical to the host restatement in frontend.py.
//
// Input: the chunks' best hypotheses (spaces removed) as ASCII bytes,
// concatenated; chunk c is bases[chunk_off[c] .. chunk_off[c+1]), read r owns
// the chunks read_off[r] .. read_off[r+1].  Empty chunks are skipped, as the
// reference drops them.  For a read's non-empty ("valid") chunks in order:
//   disp[i] = start_a - start_b of the longest common substring of chunk i-1
//             (a) and chunk i (b): the longest, then the earliest in a, then
//             the earliest in b (difflib's find_longest_match without junk);
//             la - lb when they share no character (difflib's (la, lb, 0));
//   pos[i]  = pos[i-1] + disp[i], pos[0] = 0 (may go negative);
//   length  = max(0, max over i >= 1 of pos[i] + len[i]);
//   votes   : char x of chunk i counts for class(upper(char)) in column
//             pos[i] + x (columns < 0 are dropped); classes A C G T M;
//   call    : column x < length is the class with the most votes, the lowest
//             class on a tie, A with no vote.
// difflib switches its autojunk heuristic on at len(b) >= 200, which changes
// the block it finds: a read with such a chunk is not assembled here
// (status bit 0), nor is one with a character outside ACGTM (status bit 1).
//
// Four launches on the caller's stream after two memsets (status, counts):
//   overlap: one workgroup per chunk, one thread per diagonal of the match matrix
//   place  : one workgroup per read, blocked inclusive scan of disp -> pos, length
//   vote   : one wave per chunk, integer atomics into count[5][total_bases]
//   call   : one wave per chunk's span of output columns, argmax
// A read's consensus is never longer than the sum of its chunk lengths
// (disp <= la), so read r's counts and output live at the byte offset of its
// first chunk, chunk_off[read_off[r]].
//
// With per-base weights (nd_assemble_reads_q) the same four kernels also carry
// a quality through the vote: the vote kernel adds each base's uint16 weight
// into wsum[5][total_bases] (64-bit unsigned integer atomics: the number of
// chunks on one column is not bounded, and integer sums do not depend on the
// arrival order), and the call kernel turns a column's n votes and the winning
// class's weight sum S into Q, the largest k in 0..40 with
// (double)(65535 n - S) * PHRED_RATIO[k] <= (double)(65535 n); 0 when n = 0.
//
// With per-base modification weights too (nd_assemble_reads_m, CpG models whose ninth token M is a methylated
// C) the vote kernel also adds the uint16 mw of every vote of class C or M into msum[total_bases] (one more
// 64-bit plane), and the call kernel gives a column called C or M the byte
// ML = min(255, (256 W) div (65535 n_cm)), W its msum and n_cm its C plus M votes; 0 for every other column.
//
// With per-base signal positions (nd_assemble_reads_p, the plain form's kernels with the POS flag) the vote
// kernel adds each vote's absolute position bp[.] (uint32) into psum[total_bases] (one 64-bit plane, integer
// atomics as above), the call kernel gives a column of n >= 1 votes P div n (0 with no vote), and a fifth
// launch, one workgroup per read, takes the running maximum along the read in blocks of 256 columns with a
// carry.  nd_token_positions (one launch) turns a call's attention rows into the chunk-relative positions.
//
// The four forms share one launcher: launch_assemble_reads reads the form off the optional pointer pairs of its
// AsmArgs, lays the work buffer out plane by plane (the 64-bit sums of the form, then pos, rd and the counts),
// clears the counts and the sums with one memset each, and picks the vote / call instantiations of the form.
#include "common.hpp"
#include "kernels.hpp"

namespace nd {

#define ASM_THREADS 256
#define ASM_MAXLEN 199  // longest chunk assembled here (difflib autojunk starts at 200)

// the doubles 10.0 ** (k / 10.0), k = 0..40, printed with 17 significant digits
#define ASM_PHRED_RATIOS                                                                          \
  1, 1.2589254117941673, 1.5848931924611136, 1.9952623149688795, 2.5118864315095801,              \
  3.1622776601683795, 3.9810717055349722, 5.011872336272722, 6.3095734448019334,                  \
  7.9432823472428158, 10, 12.589254117941675, 15.848931924611133, 19.952623149688797,             \
  25.118864315095795, 31.622776601683793, 39.810717055349734, 50.118723362727224,                 \
  63.095734448019329, 79.43282347242814, 100, 125.89254117941675, 158.48931924611142,             \
  199.52623149688787, 251.18864315095797, 316.22776601683796, 398.10717055349733,                 \
  501.18723362727246, 630.957344480193, 794.32823472428129, 1000, 1258.9254117941675,             \
  1584.893192461114, 1995.2623149688789, 2511.8864315095798, 3162.2776601683795,                  \
  3981.0717055349733, 5011.8723362727251, 6309.5734448019302, 7943.2823472428136, 10000
static const double h_phred_ratio[PHRED_LEVELS] = {ASM_PHRED_RATIOS};
__constant__ double d_phred_ratio[PHRED_LEVELS] = {ASM_PHRED_RATIOS};
const double* phred_ratios() { return h_phred_ratio; }

__device__ __forceinline__ int asm_class(unsigned char ch) {
  if (ch >= 'a' && ch <= 'z') ch -= 32;
  return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : ch == 'M' ? 4 : -1;
}

// the read that owns chunk c: the last r with read_off[r] <= c (reads without chunks repeat an offset)
__device__ __forceinline__ int asm_read_of(const int* __restrict__ read_off, int R, int c) {
  int lo = 0, hi = R;  // read_off[lo] <= c < read_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (read_off[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

// disp[c] and rd[c] of every chunk; status bits of its read
__global__ void __launch_bounds__(ASM_THREADS)
asm_overlap_kernel(const unsigned char* __restrict__ bases, const int* __restrict__ chunk_off,
                   const int* __restrict__ read_off, int R, int* __restrict__ disp, int* __restrict__ rd,
                   int* __restrict__ status) {
  __shared__ unsigned char sa[ASM_MAXLEN + 1], sb[ASM_MAXLEN + 1];
  __shared__ unsigned red[ASM_THREADS / 64];
  __shared__ int s_bad;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int r = asm_read_of(read_off, R, c);
  const int ob = chunk_off[c], lb = chunk_off[c + 1] - ob;
  if (tid == 0) {
    rd[c] = r;
    disp[c] = 0;
    s_bad = 0;
  }
  if (lb <= 0) return;
  if (lb > ASM_MAXLEN) {
    if (tid == 0) atomicOr(&status[r], 1);
    return;
  }
  __syncthreads();
  if (tid < lb) {
    const unsigned char ch = bases[ob + tid];
    sb[tid] = ch;
    if (asm_class(ch) < 0) s_bad = 1;
  }
  // predecessor: the nearest earlier non-empty chunk of the same read
  int p = c - 1;
  const int c0 = max(read_off[r], 0);
  while (p >= c0 && chunk_off[p + 1] - chunk_off[p] <= 0) --p;
  const int oa = p >= c0 ? chunk_off[p] : 0, la = p >= c0 ? chunk_off[p + 1] - oa : 0;
  if (la > 0 && la <= ASM_MAXLEN && tid < la) sa[tid] = bases[oa + tid];
  __syncthreads();
  if (tid == 0 && s_bad) atomicOr(&status[r], 2);
  if (la <= 0 || la > ASM_MAXLEN) return;  // a read's first valid chunk; an over-long a is flagged by its own block
  // diagonal k: i - j = k - (lb - 1); the best run on it, earliest first
  unsigned key = 0;  // len << 16 | (255 - i) << 8 | (255 - j): max = longest, then earliest in a, then in b
  for (int k = tid; k < la + lb - 1; k += ASM_THREADS) {
    const int d = k - (lb - 1);
    const int i0 = d > 0 ? d : 0, j0 = d < 0 ? -d : 0;
    const int n = min(la - i0, lb - j0);
    int run = 0, best = 0, bs = 0;
    for (int s = 0; s < n; ++s) {
      run = sa[i0 + s] == sb[j0 + s] ? run + 1 : 0;
      if (run > best) {
        best = run;
        bs = s - run + 1;
      }
    }
    if (best > 0) {
      const unsigned kk = ((unsigned)best << 16) | ((unsigned)(255 - (i0 + bs)) << 8) | (unsigned)(255 - (j0 + bs));
      key = max(key, kk);
    }
  }
  for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < ASM_THREADS / 64; ++w) key = max(key, red[w]);
    disp[c] = key ? (255 - (int)((key >> 8) & 255u)) - (255 - (int)(key & 255u)) : la - lb;
  }
}

// pos[c] = inclusive scan of disp over the read's chunks (in place), seq_len[r]
__global__ void __launch_bounds__(ASM_THREADS)
asm_place_kernel(const int* __restrict__ chunk_off, const int* __restrict__ read_off, int* __restrict__ pos,
                 const int* __restrict__ status, int* __restrict__ seq_len) {
  __shared__ int sd[ASM_THREADS], sn[ASM_THREADS], smax[ASM_THREADS];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (status[r] != 0) {
    if (tid == 0) seq_len[r] = -1;
    return;
  }
  const int c0 = read_off[r], c1 = read_off[r + 1];
  int carry_d = 0, carry_n = 0, best = 0;  // best: max(0, pos + len) over this thread's valid chunks i >= 1
  for (int base = c0; base < c1; base += ASM_THREADS) {
    const int c = base + tid;
    const int len = c < c1 ? chunk_off[c + 1] - chunk_off[c] : 0;
    sd[tid] = c < c1 ? pos[c] : 0;
    sn[tid] = len > 0 ? 1 : 0;
    __syncthreads();
    for (int o = 1; o < ASM_THREADS; o <<= 1) {
      const int ad = tid >= o ? sd[tid - o] : 0, an = tid >= o ? sn[tid - o] : 0;
      __syncthreads();
      sd[tid] += ad;
      sn[tid] += an;
      __syncthreads();
    }
    const int pc = carry_d + sd[tid], nc = carry_n + sn[tid];
    if (c < c1) pos[c] = pc;
    if (len > 0 && nc > 1) best = max(best, pc + len);
    carry_d += sd[ASM_THREADS - 1];
    carry_n += sn[ASM_THREADS - 1];
    __syncthreads();
  }
  smax[tid] = best;
  __syncthreads();
  for (int s = ASM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) smax[tid] = max(smax[tid], smax[tid + s]);
    __syncthreads();
  }
  if (tid == 0) seq_len[r] = smax[0];
}

// one wave per chunk: its chars vote at pos[c] + x of the read's columns; QUAL: each vote's weight qw[.] is
// added to wsum of its class and column; MOD: a C or M vote's modification weight mw[.] to msum of its column;
// POS: each vote's absolute signal position bp[.] to psum of its column
template <bool QUAL, bool MOD = false, bool POS = false>
__global__ void __launch_bounds__(ASM_THREADS)
asm_vote_kernel(const unsigned char* __restrict__ bases, const unsigned short* __restrict__ qw,
                const unsigned short* __restrict__ mw, const int* __restrict__ chunk_off,
                const int* __restrict__ read_off, const int* __restrict__ pos, const int* __restrict__ rd,
                const int* __restrict__ status, int C, int total, int* __restrict__ count,
                unsigned long long* __restrict__ wsum, unsigned long long* __restrict__ msum,
                const unsigned* __restrict__ bp, unsigned long long* __restrict__ psum) {
  const int c = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const int r = rd[c];
  if (status[r] != 0) return;
  const int o = chunk_off[c], len = chunk_off[c + 1] - o, p = pos[c];
  const int r0 = chunk_off[read_off[r]], cols = chunk_off[read_off[r + 1]] - r0;
  for (int x = lane; x < len; x += 64) {
    const int col = p + x, cls = asm_class(bases[o + x]);
    if (col >= 0 && col < cols && r0 + col < total && cls >= 0) {
      atomicAdd(&count[(size_t)cls * total + r0 + col], 1);
      if (QUAL) atomicAdd(&wsum[(size_t)cls * total + r0 + col], (unsigned long long)qw[o + x]);
      if (MOD && (cls == 1 || cls == 4)) atomicAdd(&msum[r0 + col], (unsigned long long)mw[o + x]);
      if (POS) atomicAdd(&psum[r0 + col], (unsigned long long)bp[o + x]);
    }
  }
}

// one wave per chunk's span of the output: column g - r0 of read rd[c], 0 past the read's length; QUAL: the
// column's Q from its votes and the winning class's weight sum; MOD: ML of a column called C or M from its C
// and M votes and their modification weight sum; POS: the column's position, its votes' position sum over
// their number (asm_pos_scan_kernel then makes the positions monotone along the read)
template <bool QUAL, bool MOD = false, bool POS = false>
__global__ void __launch_bounds__(ASM_THREADS)
asm_call_kernel(const int* __restrict__ chunk_off, const int* __restrict__ read_off, const int* __restrict__ rd,
                const int* __restrict__ seq_len, const int* __restrict__ count,
                const unsigned long long* __restrict__ wsum, const unsigned long long* __restrict__ msum, int C,
                int total, unsigned char* __restrict__ seq, unsigned char* __restrict__ qual,
                unsigned char* __restrict__ ml, const unsigned long long* __restrict__ psum,
                unsigned* __restrict__ rpos) {
  const int c = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const int r = rd[c];
  const int o = chunk_off[c], len = chunk_off[c + 1] - o;
  const int r0 = chunk_off[read_off[r]], n = seq_len[r];
  for (int x = lane; x < len; x += 64) {
    const int g = o + x;
    if (g >= total) break;
    unsigned char out = 0, q = 0, mod = 0;
    unsigned cp = 0;
    if (g - r0 < n) {
      int best = count[g], cls = 0;
      long long votes = best;
      for (int k = 1; k < 5; ++k) {
        const int v = count[(size_t)k * total + g];
        votes += v;
        if (v > best) {
          best = v;
          cls = k;
        }
      }
      out = (unsigned char)((0x4D54474341ull >> (8 * cls)) & 0xFFu);  // "ACGTM"[cls]
      if (QUAL && votes > 0) {
        const unsigned long long full = 65535ull * (unsigned long long)votes;
        const double e = (double)(full - wsum[(size_t)cls * total + g]), f = (double)full;  // both exact
        for (int k = 1; k < PHRED_LEVELS && e * d_phred_ratio[k] <= f; ++k) q = (unsigned char)k;
      }
      if (POS && votes > 0) cp = (unsigned)(psum[g] / (unsigned long long)votes);  // a mean of uint32 values
      if (MOD && (cls == 1 || cls == 4)) {
        const unsigned long long n_cm =
            (unsigned long long)count[(size_t)total + g] + (unsigned long long)count[(size_t)4 * total + g];
        if (n_cm > 0) {  // W <= 65535 n_cm < 2^47: 256 W fits
          const unsigned long long v = (256ull * msum[g]) / (65535ull * n_cm);
          mod = (unsigned char)(v < 255ull ? v : 255ull);
        }
      }
    }
    seq[g] = out;
    if (QUAL) qual[g] = q;
    if (MOD) ml[g] = mod;
    if (POS) rpos[g] = cp;
  }
}

// rpos of read r, in place: the running maximum of its column positions, r[x] = max(r[x-1], col[x]) over its
// seq_len[r] columns, in blocks of ASM_THREADS columns with a carry (as asm_place_kernel scans disp)
__global__ void __launch_bounds__(ASM_THREADS)
asm_pos_scan_kernel(const int* __restrict__ chunk_off, const int* __restrict__ read_off,
                    const int* __restrict__ seq_len, int total, unsigned* __restrict__ rpos) {
  __shared__ unsigned sm[ASM_THREADS];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int r0 = chunk_off[read_off[r]];
  // a read's columns are its own bytes
  const int n = min(min(seq_len[r], chunk_off[read_off[r + 1]] - r0), total - r0);
  unsigned carry = 0;
  for (int base = 0; base < n; base += ASM_THREADS) {
    const int x = base + tid;
    sm[tid] = x < n ? rpos[r0 + x] : 0u;
    __syncthreads();
    for (int o = 1; o < ASM_THREADS; o <<= 1) {
      const unsigned a = tid >= o ? sm[tid - o] : 0u;
      __syncthreads();
      sm[tid] = max(sm[tid], a);
      __syncthreads();
    }
    if (x < n) rpos[r0 + x] = max(carry, sm[tid]);
    carry = max(carry, sm[ASM_THREADS - 1]);
    __syncthreads();
  }
}

// the 64-bit planes of a form: wsum's five, msum's one, psum's one
static size_t asm_planes64(bool qual, bool mod, bool pos) { return (qual ? 5 : 0) + (mod ? 1 : 0) + (pos ? 1 : 0); }

size_t assemble_work_bytes(int C, long long total, bool qual, bool mod, bool pos) {
  return asm_planes64(qual, mod, pos) * (size_t)total * sizeof(unsigned long long) + (size_t)2 * C * sizeof(int) +
         (size_t)5 * total * sizeof(int);
}

hipError_t launch_assemble_reads(const AsmArgs& a, hipStream_t s) {
  const bool q = a.qual != nullptr, m = a.ml != nullptr, p = a.rpos != nullptr;  // the form: which pairs are given
  const int R = a.R, C = a.C, total = a.total;
  if (R < 0 || C < 0 || total < 0 || !a.chunk_off || !a.read_off || (R > 0 && (!a.seq_len || !a.status)) ||
      (C > 0 && !a.work) || (total > 0 && (!a.bases || !a.seq)) || (a.qw != nullptr) != q ||
      (a.mw != nullptr) != m || (m && !q) || (a.bp != nullptr) != p || (p && q))
    return hipErrorInvalidValue;
  if (R == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.status, 0, (size_t)R * sizeof(int), s);
  if (e != hipSuccess) return e;
  if (C == 0) return hipMemsetAsync(a.seq_len, 0, (size_t)R * sizeof(int), s);  // no chunks: every read is ""
  // work, plane by plane: the 64-bit sums first, so they are 8-byte aligned whatever C is (wsum[5][total],
  // msum[total], psum[total], each only in its form), then pos[C], rd[C] and count[5][total]
  unsigned long long* const sums = static_cast<unsigned long long*>(a.work);
  unsigned long long* next = sums;
  auto plane = [&](bool on, int n) {
    unsigned long long* at = on ? next : nullptr;
    if (on) next += (size_t)n * total;
    return at;
  };
  unsigned long long* wsum = plane(q, 5);
  unsigned long long* msum = plane(m, 1);
  unsigned long long* psum = plane(p, 1);
  int* pos = reinterpret_cast<int*>(next);
  int* rd = pos + C;
  int* count = rd + C;
  if (total > 0) {
    e = hipMemsetAsync(count, 0, (size_t)5 * total * sizeof(int), s);
    if (e == hipSuccess && next != sums) e = hipMemsetAsync(sums, 0, (size_t)(next - sums) * sizeof(*sums), s);
    if (e != hipSuccess) return e;
  }
  const int per = ASM_THREADS / 64;
  const dim3 grid((C + per - 1) / per), block(ASM_THREADS);
  hipLaunchKernelGGL(asm_overlap_kernel, dim3(C), block, 0, s, a.bases, a.chunk_off, a.read_off, R, pos, rd, a.status);
  hipLaunchKernelGGL(asm_place_kernel, dim3(R), block, 0, s, a.chunk_off, a.read_off, pos, a.status, a.seq_len);
  auto go = [&](auto vote, auto call) {
    hipLaunchKernelGGL(vote, grid, block, 0, s, a.bases, a.qw, a.mw, a.chunk_off, a.read_off, pos, rd, a.status, C,
                       total, count, wsum, msum, a.bp, psum);
    hipLaunchKernelGGL(call, grid, block, 0, s, a.chunk_off, a.read_off, rd, a.seq_len, count, wsum, msum, C, total,
                       a.seq, a.qual, a.ml, psum, a.rpos);
  };
  if (total == 0) return hipGetLastError();  // only empty chunks: place has written every seq_len
  if (m)
    go(asm_vote_kernel<true, true>, asm_call_kernel<true, true>);
  else if (q)
    go(asm_vote_kernel<true>, asm_call_kernel<true>);
  else if (p)
    go(asm_vote_kernel<false, false, true>, asm_call_kernel<false, false, true>);
  else
    go(asm_vote_kernel<false>, asm_call_kernel<false>);
  if (p)
    hipLaunchKernelGGL(asm_pos_scan_kernel, dim3(R), block, 0, s, a.chunk_off, a.read_off, a.seq_len, total, a.rpos);
  return hipGetLastError();
}

// w[i] = the token weight of tokens[i]: min(65535, floor(65535 exp((double)lp) + 0.5)) of its log-prob lp
// (logp[i][tokens[i]], or tok_logp[i]); 0 for a token outside [0, V) or a non-finite lp
#define TW_THREADS 256
__global__ void __launch_bounds__(TW_THREADS)
token_weights_kernel(const int* __restrict__ tokens, const float* __restrict__ logp,
                     const float* __restrict__ tok_logp, int n, int V, unsigned short* __restrict__ w) {
  const int i = blockIdx.x * TW_THREADS + threadIdx.x;
  if (i >= n) return;
  const int t = tokens[i];
  unsigned short out = 0;
  if (t >= 0 && t < V) {
    const float lp = logp ? logp[(size_t)i * V + t] : tok_logp[i];
    if (isfinite(lp)) {
      const double x = floor(__dadd_rn(__dmul_rn(65535.0, exp((double)lp)), 0.5));  // a product, then a sum: no FMA
      out = (unsigned short)(x < 65535.0 ? x : 65535.0);
    }
  }
  w[i] = out;
}

hipError_t launch_token_weights(const int* tokens, const float* logp, const float* tok_logp, int n, int V,
                                unsigned short* w, hipStream_t s) {
  if (n < 0 || V < 1 || (n > 0 && (!tokens || !w)) || (logp != nullptr) == (tok_logp != nullptr))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(token_weights_kernel, dim3((n + TW_THREADS - 1) / TW_THREADS), dim3(TW_THREADS), 0, s, tokens,
                     logp, tok_logp, n, V, w);
  return hipGetLastError();
}

// mw[i] = the modification weight of tokens[i] from its step's log-probs lp = logp[i]: 0 unless the token is
// canon (C) or mod (M); else with d = (double)lp[canon] - (double)lp[mod], min(65535, floor(65535 / (1 + exp(d)) +
// 0.5)), every operation rounded once (no FMA); a NaN d falls back to the hard call (65535 for mod, 0 for canon)
__global__ void __launch_bounds__(TW_THREADS)
token_mod_weights_kernel(const int* __restrict__ tokens, const float* __restrict__ logp, int n, int V, int canon,
                         int mod, unsigned short* __restrict__ mw) {
  const int i = blockIdx.x * TW_THREADS + threadIdx.x;
  if (i >= n) return;
  const int t = tokens[i];
  unsigned short out = 0;
  if (t == canon || t == mod) {  // both inside [0, V): the launcher checked
    const double d = __dsub_rn((double)logp[(size_t)i * V + canon], (double)logp[(size_t)i * V + mod]);
    if (d != d) {
      out = t == mod ? 65535 : 0;
    } else {
      const double p = __ddiv_rn(1.0, __dadd_rn(1.0, exp(d)));  // exp(+inf) = inf -> 0, exp(-inf) = 0 -> 1
      const double x = floor(__dadd_rn(__dmul_rn(65535.0, p), 0.5));
      out = (unsigned short)(x < 65535.0 ? x : 65535.0);
    }
  }
  mw[i] = out;
}

hipError_t launch_token_mod_weights(const int* tokens, const float* logp, int n, int V, int canon, int mod,
                                    unsigned short* mw, hipStream_t s) {
  if (n < 0 || V < 1 || canon < 0 || canon >= V || mod < 0 || mod >= V || canon == mod ||
      (n > 0 && (!tokens || !logp || !mw)))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(token_mod_weights_kernel, dim3((n + TW_THREADS - 1) / TW_THREADS), dim3(TW_THREADS), 0, s,
                     tokens, logp, n, V, canon, mod, mw);
  return hipGetLastError();
}

// pos[b][s] = m[s] of chunk b: the centroid c[s] = (2 M + Q) div (2 Q) of attention row s over t < min(span[b],
// T), with q_t = 0 unless a[t] > 0, 2^24 when a[t] >= 1, else floor((double)a[t] * 2^24 + 0.5), Q = sum q_t and
// M = sum q_t t in 64-bit integers (c = 0 when Q = 0), then m[s] = max(m[s-1], c[s]).  One workgroup per chunk:
// the waves take the rows of a block of TP_THREADS steps, the lanes stride over t, Q and M are reduced over the
// wave, c goes to LDS, and the block is max-scanned with a carry.
#define TP_THREADS 256
__global__ void __launch_bounds__(TP_THREADS)
token_positions_kernel(const float* __restrict__ attn, long long ld_chunk, const int* __restrict__ span, int S, int T,
                       int* __restrict__ pos) {
  __shared__ int sc[TP_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = min(max(span[b], 0), T);
  const float* a0 = attn + (size_t)b * (size_t)ld_chunk;
  int carry = 0;
  for (int base = 0; base < S; base += TP_THREADS) {
    const int rows = min(TP_THREADS, S - base);
    sc[tid] = 0;
    __syncthreads();
    for (int i = wave; i < rows; i += TP_THREADS / 64) {
      const float* a = a0 + (size_t)(base + i) * T;
      unsigned long long Q = 0, M = 0;
      for (int t = lane; t < n; t += 64) {
        const float v = a[t];
        unsigned long long q = 0;
        if (v > 0.f)  // false for NaN, negatives and -0
          q = v >= 1.f ? 1ull << 24 : (unsigned long long)floor((double)v * 16777216.0 + 0.5);  // exact in fp64
        Q += q;
        M += q * (unsigned long long)t;
      }
      for (int o = 32; o > 0; o >>= 1) {
        Q += __shfl_xor(Q, o, 64);
        M += __shfl_xor(M, o, 64);
      }
      if (lane == 0) sc[i] = Q ? (int)((2 * M + Q) / (2 * Q)) : 0;
    }
    __syncthreads();
    for (int o = 1; o < TP_THREADS; o <<= 1) {
      const int v = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] = max(sc[tid], v);
      __syncthreads();
    }
    if (tid < rows) pos[(size_t)b * S + base + tid] = max(carry, sc[tid]);
    carry = max(carry, sc[TP_THREADS - 1]);
    __syncthreads();
  }
}

hipError_t launch_token_positions(const float* attn, long long ld_chunk, const int* span, int B, int S, int T,
                                  int* pos, hipStream_t s) {
  if (B < 0 || S < 0 || T < 1 || T > TOKEN_POS_MAX_T || ld_chunk < (long long)S * T ||
      (long long)B * S >= 1ll << 31 || (B > 0 && !span) || ((long long)B * S > 0 && (!attn || !pos)))
    return hipErrorInvalidValue;
  if (B == 0 || S == 0) return hipSuccess;
  hipLaunchKernelGGL(token_positions_kernel, dim3(B), dim3(TP_THREADS), 0, s, attn, ld_chunk, span, S, T, pos);
  return hipGetLastError();
}

}  // namespace nd
