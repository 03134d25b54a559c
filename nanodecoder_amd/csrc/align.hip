// Global alignment of called reads to their known sequences on the device (nd_align_seqs): the edit-distance
// DP of every pair with a fixed tie rule, exactly the host rule of nanodecoder_amd/accuracy.py (align_host).
// The reference measures read accuracy outside its own code (minimap2, then matches over alignment length);
// there is no reference equivalent of this file.
//
// The rule.  Call a[0..n), truth b[0..m), bytes compared for equality (the caller normalises them).
//   borders    : D[i][0] = i, D[0][j] = j;
//   recurrence : D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1);
//   direction at (i, j), taken in this order:
//     diagonal if i, j >= 1 and D[i-1][j-1] + (a[i-1] != b[j-1]) == D[i][j];
//     else up  if i >= 1 and (j == 0 or D[i-1][j] + 1 == D[i][j]): consumes a[i-1] only, an inserted base;
//     else left: consumes b[j-1] only, a base missing from the call;
//   alignment  : the path those directions give from (n, m) back to (0, 0);
//   per call base op[i]: 0 = match, 1 = mismatch (both diagonal steps), 2 = insertion (an up step);
//   per pair five int32 {dist, n_match, n_sub, n_ins, n_del}: n_match + n_sub + n_ins == n,
//     n_match + n_sub + n_del == m, dist == n_sub + n_ins + n_del == D[n][m].
//
// Two launches on the caller's stream:
//   offsets: one workgroup, a blocked scan of the pairs' direction bytes -> 64-bit offsets in the work buffer
//   align  : one workgroup of 256 threads per pair, the DP and then the traceback
//
// The DP.  A thread owns ALN_ROWS = 4 consecutive rows of a strip of 1024 rows and walks them in blocks of 16
// columns; thread t works on block g - t at step g (a skewed strip: the blocks of one anti-diagonal of the
// thread x block grid run in parallel), and the strips are chained: thread 0 starts the next strip's block 0
// max(blocks, 256) steps after this strip's.  One barrier per step.  A thread's frontier is in registers (the
// 16 + 1 values above its block, the 4 values left of it); what crosses threads is in LDS as uint16 (distances
// stay below 2^15): the bottom row of a thread's block for the thread below (double buffered by the step's
// parity), and the bottom row of the strip, which thread 255 writes and thread 0 reads one strip later, in
// place (a block is read 256 or more steps after it is written and rewritten 255 steps after it is read).
// Both sequences are in LDS.  Only the 2-bit directions (0 diagonal, 1 up, 2 left) go to global memory: a row
// of a block is one full 32-bit word, stored by the one thread that owns the row (no races).
//
// The directions of a pair with W = m div 16 full blocks and r = m mod 16 columns left over:
//   word (i - 1) * W + blk              : columns 16 blk + 1 .. 16 blk + 16 of row i, column c at bits 2 (c mod 16)
//   then ceil(n r / 4) bytes            : the rows' last r columns; rows 4 q + 1 .. 4 q + 4 (one thread's) are the
//                                         r bytes at q r, row k of them at bits 2 k r, column by column
// rounded up to 4 bytes: at most n m / 4 + 4 bytes.  The work buffer holds the P + 1 offsets (8 bytes each), then
// the pairs' directions; nd_align_seqs_work_bytes(P, cells) = cells div 4 + 16 P + 64 covers both.  A pair fits
// when its directions end inside the bytes that bound leaves for them (whatever larger buffer the caller passed:
// the result does not depend on the buffer's size).
//
// The traceback.  The 256 threads load a window of the directions, 64 rows by 4 blocks ending at the path's
// cell, into LDS; thread 0 walks the path inside it (writing op[] and counting), and the window moves.  A border
// ends it: the rest of a column 0 is insertions (written by all threads), the rest of row 0 deletions.
//
// The fit form (nd_align_fit, FIT = true below; the rule is in nanodecoder_amd/accuracy.py, fit_host): the truth
// of pair p is the window ref[hit[p][1] .. hit[p][2]) of one shared reference and its ends are free: D[0][j] = 0
// (the strip row starts at 0), the alignment ends in the smallest j* with D[n][j*] minimal and its path runs from
// (n, j*) until i == 0, nothing consumed on row 0.  Row n lies in the last strip, whose bottom row no strip reads:
// there the thread that owns row n, and no other, writes into the strip row, and what it writes is row n, block by
// block (the loop is instantiated for each of the four places row n can have among its rows); after the DP all
// threads reduce (D[n][j], j) over j = 0..m (D[n][0] = n, the padded columns j > m left out) to the smallest key.  A pair whose status has bit 0 set on entry (unmapped) is skipped.  The global
// form's instantiation holds none of this.
//
// The pos form (nd_align_fit_pos, POS = true): the fit form with one more output, rpos[i] = the reference position
// of oriented call base i in ref's coordinates.  The traceback is where j is known: a diagonal step at cell
// (i + 1, j) and an up step at column j both give w0 + j - 1 (the base matched or mismatched to, and the base to
// the left of an inserted one), the column-0 border gives w0 - 1, and a pair that is not aligned gives -1.  Only
// stores next to those of op[]: the other instantiations hold none of it.
//
// LDS: 2 x 8208 (sequences) + 16416 (strip row) + 16384 (block rows) + 1024 (window) + 8 = 50,248 bytes static
// (the fit form: + 4).
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

namespace nd {

#define ALN_THREADS 256
#define ALN_ROWS 4
#define ALN_STRIP (ALN_THREADS * ALN_ROWS)
#define ALN_WIN_ROWS 64
#define ALN_WIN_BLKS 4

// direction bytes of an n x m pair (0 for one that is not aligned here, or has an empty side)
__host__ __device__ __forceinline__ long long aln_pair_bytes(int n, int m) {
  if (n <= 0 || m <= 0 || n > ALIGN_MAX_LEN || m > ALIGN_MAX_LEN) return 0;
  const long long b = 4ll * n * (m >> 4) + ((long long)n * (m & 15) + 3) / 4;
  return (b + 3) & ~3ll;
}

// pair p's sides.  Global form: tb = truth_off.  Fit form: tb = hit [P, 4], the truth the window hit[p][1] ..
// hit[p][2] of a reference of ref_len bytes.  Returns 0, or the fit form's 1 = skipped (status bit 0 on entry),
// 4 = the window is not inside [0, ref_len]
template <bool FIT>
__device__ __forceinline__ int aln_dims(const int* __restrict__ call_off, const int* __restrict__ tb,
                                        const int* __restrict__ status, int ref_len, int p, int& n, int& ob, int& m) {
  n = call_off[p + 1] - call_off[p];
  if constexpr (FIT) {
    ob = tb[4 * (size_t)p + 1];
    m = tb[4 * (size_t)p + 2] - ob;
    if (status[p] & 1) return 1;
    if (ob < 0 || m < 0 || (long long)ob + m > ref_len) return 4;
  } else {
    ob = tb[p];
    m = tb[p + 1] - ob;
  }
  return 0;
}

// off[p] = the direction bytes of the pairs before p, off[P] their total: a blocked scan with a carry
template <bool FIT>
__global__ void __launch_bounds__(ALN_THREADS)
align_offsets_kernel(const int* __restrict__ call_off, const int* __restrict__ truth_off, int P,
                     long long* __restrict__ off, const int* __restrict__ status, int ref_len) {
  __shared__ long long sm[ALN_THREADS];
  const int tid = threadIdx.x;
  long long carry = 0;
  for (int base = 0; base < P; base += ALN_THREADS) {
    const int p = base + tid;
    long long mine = 0;
    if (p < P) {
      int n, ob, m;
      if (aln_dims<FIT>(call_off, truth_off, status, ref_len, p, n, ob, m) == 0) mine = aln_pair_bytes(n, m);
    }
    sm[tid] = mine;
    __syncthreads();
    for (int o = 1; o < ALN_THREADS; o <<= 1) {
      const long long v = tid >= o ? sm[tid - o] : 0;
      __syncthreads();
      sm[tid] += v;
      __syncthreads();
    }
    if (p < P) off[p] = carry + sm[tid] - mine;
    carry += sm[ALN_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) off[P] = carry;
}

// the direction word of block blk of row i (columns 16 blk + 1 ..; column c at bits 2 (c mod 16))
__device__ __forceinline__ unsigned aln_dir_word(const unsigned* __restrict__ full, const unsigned char* __restrict__ rem,
                                                 long long rem_bytes, int W, int r, int i, int blk) {
  if (blk < W) return full[(i - 1) * W + blk];
  const int q = (i - 1) >> 2, bit0 = ((i - 1) & 3) * r * 2;
  const long long b0 = (long long)q * r + (bit0 >> 3);
  unsigned long long v = 0;
#pragma unroll
  for (int x = 0; x < 5; ++x)
    if (b0 + x < rem_bytes) v |= (unsigned long long)rem[b0 + x] << (8 * x);
  return (unsigned)(v >> (bit0 & 7)) & ((1u << (2 * r)) - 1u);
}

template <bool FIT, bool POS>
__global__ void __launch_bounds__(ALN_THREADS)
align_kernel(const unsigned char* __restrict__ call, const int* __restrict__ call_off,
             const unsigned char* __restrict__ truth, const int* __restrict__ truth_off,
             const long long* __restrict__ off, long long capacity, unsigned char* __restrict__ dirs,
             int* __restrict__ counts, unsigned char* __restrict__ ops, int* __restrict__ status,
             int* __restrict__ span, int ref_len, int* __restrict__ rpos) {
  static_assert(FIT || !POS, "positions belong to the fit form");
  __shared__ __align__(16) unsigned char sa[ALIGN_MAX_LEN + 16], sb[ALIGN_MAX_LEN + 16];
  __shared__ __align__(16) unsigned short srow[ALIGN_MAX_LEN + 16];  // srow[j - 1] = D[the strip's top row][j]
  __shared__ __align__(16) unsigned short sx[2][ALN_THREADS][16];    // [step parity][thread]: its block's bottom row
  __shared__ unsigned swin[ALN_WIN_ROWS][ALN_WIN_BLKS];
  __shared__ int s_ij[2];
  __shared__ int s_end[1];  // the fit form: j*
  const int p = blockIdx.x, tid = threadIdx.x;
  const int oa = call_off[p];
  int n, ob, m;
  const int dims = aln_dims<FIT>(call_off, truth_off, status, ref_len, p, n, ob, m);
  unsigned char* op = ops ? ops + oa : nullptr;
  int* rp = POS ? rpos + oa : nullptr;  // the pos form: the reference position of every oriented call base
  int bad = 0;
  if (FIT && dims) bad = dims;
  else if (n < 0 || m < 0 || n > ALIGN_MAX_LEN || m > ALIGN_MAX_LEN) bad = FIT ? 4 : 1;
  else if (off[p + 1] > capacity) bad = 2;
  if (bad) {
    if (tid == 0 && !(FIT && bad == 1)) status[p] = bad;  // a skipped pair keeps its status
    if (tid < 5) counts[(size_t)p * 5 + tid] = -1;
    if (FIT && tid < 2) span[(size_t)p * 2 + tid] = -1;
    if (op)
      for (int x = tid; x < n; x += ALN_THREADS) op[x] = 0;
    if constexpr (POS)
      for (int x = tid; x < n; x += ALN_THREADS) rp[x] = -1;
    return;
  }
  if (tid == 0) status[p] = 0;
  const int W = m >> 4, r = m & 15, mb = (m + 15) >> 4;
  const int nstrips = (n + ALN_STRIP - 1) / ALN_STRIP;
  const long long rem_bytes = ((long long)n * r + 3) / 4;
  unsigned* full = reinterpret_cast<unsigned*>(dirs + off[p]);
  unsigned char* rem = dirs + off[p] + 4ll * n * W;
  if (n > 0 && m > 0) {
    for (int x = tid; x < nstrips * ALN_STRIP; x += ALN_THREADS) sa[x] = x < n ? call[oa + x] : 0;
    for (int x = tid; x < mb * 16; x += ALN_THREADS) {
      sb[x] = x < m ? truth[ob + x] : 0;
      srow[x] = FIT ? (unsigned short)0 : (unsigned short)(x + 1);
    }
    __syncthreads();
    const int period = max(mb, ALN_THREADS);           // steps between two strips' block 0 on one thread
    const int steps = nstrips * period + ALN_THREADS;  // thread 255's last block is step (nstrips-1) period + mb + 254
    // the fit form: row n lies in the last strip, whose bottom row nobody reads; there the thread that owns row n
    // writes that row into the strip row and no other thread does (thread 0 has read a block of it at least one
    // step before the owner writes there).  Which of the owner's four rows it is, is the same for the whole pair:
    // the loop is instantiated per value (own_k below), so that the row is picked at compile time
    const bool own = FIT && tid == ((n - 1) % ALN_STRIP) / ALN_ROWS;
    auto dp = [&](auto own_k_c) {
    constexpr int OWN_K = decltype(own_k_c)::value;
    int left[ALN_ROWS], corner = 0;
    int s = 0, cb = -tid;  // this thread's strip and block at the current step (cb < 0: not started)
    for (int g = 0; g < steps; ++g) {
      if (cb >= 0 && cb < mb && s < nstrips) {
        const int i0 = s * ALN_STRIP + tid * ALN_ROWS + 1;  // the first of this thread's rows
        if (cb == 0) {
#pragma unroll
          for (int k = 0; k < ALN_ROWS; ++k) left[k] = i0 + k;
          corner = i0 - 1;
        }
        // the row above the block: the strip's top row for thread 0, else the block row of the thread above
        const uint4* src = reinterpret_cast<const uint4*>(tid == 0 ? &srow[16 * cb] : &sx[(g - 1) & 1][tid - 1][0]);
        const uint4 t0 = src[0], t1 = src[1];
        const unsigned tw[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        int top[17];
        top[0] = corner;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          top[2 * c + 1] = (int)(tw[c] & 0xFFFFu);
          top[2 * c + 2] = (int)(tw[c] >> 16);
        }
        corner = top[16];  // D[i0 - 1][16 (cb + 1)]: the next block's corner
        const uint4 bq = *reinterpret_cast<const uint4*>(&sb[16 * cb]);
        const unsigned bw[4] = {bq.x, bq.y, bq.z, bq.w};
        const unsigned aw = *reinterpret_cast<const unsigned*>(&sa[i0 - 1]);
        unsigned words[ALN_ROWS];
        const bool last_strip = FIT && s == nstrips - 1;
        unsigned rown[8];  // the fit form: row OWN_K of this block, packed like the bottom row
#pragma unroll
        for (int k = 0; k < ALN_ROWS; ++k) {
          const int ai = (int)((aw >> (8 * k)) & 0xFFu);
          int diag = top[0], lft = left[k];
          top[0] = lft;
          unsigned word = 0;
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const int bj = (int)((bw[c >> 2] >> (8 * (c & 3))) & 0xFFu);
            const int up = top[c + 1];
            const int d1 = diag + (ai != bj ? 1 : 0), d2 = up + 1, d3 = lft + 1;
            const int v = min(d1, min(d2, d3));
            const unsigned dir = d1 == v ? 0u : d2 == v ? 1u : 2u;
            word |= dir << (2 * c);
            diag = up;
            top[c + 1] = v;
            lft = v;
          }
          left[k] = lft;
          words[k] = word;
          if constexpr (FIT) {
            if (k == OWN_K && OWN_K < ALN_ROWS - 1) {  // (folds once k is unrolled) for the owner, D[n][16 cb + 1 ..]
#pragma unroll
              for (int c = 0; c < 8; ++c) rown[c] = (unsigned)top[2 * c + 1] | ((unsigned)top[2 * c + 2] << 16);
            }
          }
        }
        uint4 o0, o1;
        o0.x = (unsigned)top[1] | ((unsigned)top[2] << 16);
        o0.y = (unsigned)top[3] | ((unsigned)top[4] << 16);
        o0.z = (unsigned)top[5] | ((unsigned)top[6] << 16);
        o0.w = (unsigned)top[7] | ((unsigned)top[8] << 16);
        o1.x = (unsigned)top[9] | ((unsigned)top[10] << 16);
        o1.y = (unsigned)top[11] | ((unsigned)top[12] << 16);
        o1.z = (unsigned)top[13] | ((unsigned)top[14] << 16);
        o1.w = (unsigned)top[15] | ((unsigned)top[16] << 16);
        if constexpr (FIT && OWN_K < ALN_ROWS - 1) {
          // the owner stores row n in place of its bottom row: the threads below it hold rows past n, whose values
          // reach no output (their directions are not stored, and the strip row takes nothing from them here)
          const bool mine = own && last_strip;
          o0.x = mine ? rown[0] : o0.x;
          o0.y = mine ? rown[1] : o0.y;
          o0.z = mine ? rown[2] : o0.z;
          o0.w = mine ? rown[3] : o0.w;
          o1.x = mine ? rown[4] : o1.x;
          o1.y = mine ? rown[5] : o1.y;
          o1.z = mine ? rown[6] : o1.z;
          o1.w = mine ? rown[7] : o1.w;
        }
        // one store, its destination selected: a second store under a condition of its own made hipcc keep 279
        // registers live here instead of 97
        uint4* dst = reinterpret_cast<uint4*>((last_strip ? own : tid == ALN_THREADS - 1) ? &srow[16 * cb]
                                                                                         : &sx[g & 1][tid][0]);
        dst[0] = o0;
        dst[1] = o1;
        if (cb < W) {
#pragma unroll
          for (int k = 0; k < ALN_ROWS; ++k)
            if (i0 + k <= n) full[(i0 + k - 1) * W + cb] = words[k];
        } else {  // the last r columns of this thread's four rows: r bytes of its own
          const unsigned mask = (1u << (2 * r)) - 1u;
          unsigned __int128 v = 0;
#pragma unroll
          for (int k = 0; k < ALN_ROWS; ++k) v |= (unsigned __int128)(words[k] & mask) << (2 * r * k);
          const long long b0 = (long long)((i0 - 1) >> 2) * r;
          const int nb = (int)min((long long)r, rem_bytes - b0);
          for (int x = 0; x < nb; ++x) rem[b0 + x] = (unsigned char)(v >> (8 * x));
        }
      }
      if (++cb == period) {
        cb = 0;
        ++s;
      }
      __syncthreads();
    }
    };
    if constexpr (FIT) {
      switch ((n - 1) % ALN_ROWS) {
        case 0: dp(std::integral_constant<int, 0>{}); break;
        case 1: dp(std::integral_constant<int, 1>{}); break;
        case 2: dp(std::integral_constant<int, 2>{}); break;
        default: dp(std::integral_constant<int, ALN_ROWS - 1>{}); break;
      }
    } else {
      dp(std::integral_constant<int, ALN_ROWS - 1>{});
    }
    __threadfence();  // the directions, before other threads of the workgroup read them back
    if constexpr (FIT) {  // the smallest j with D[n][j] minimal: srow[j - 1] = D[n][j], D[n][0] = n; (value, j) as one key
      unsigned best = (unsigned)n << 14;
      for (int j = tid + 1; j <= m; j += ALN_THREADS) best = min(best, ((unsigned)srow[j - 1] << 14) | (unsigned)j);
      unsigned* red = &swin[0][0];  // 256 words, free until the traceback
      red[tid] = best;
      __syncthreads();
      for (int o = ALN_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = min(red[tid], red[tid + o]);
        __syncthreads();
      }
      if (tid == 0) s_end[0] = (int)(red[0] & 0x3FFFu);
    }
  } else if constexpr (FIT) {
    if (tid == 0) s_end[0] = 0;  // an empty side: j* = 0
  }
  if constexpr (FIT) __syncthreads();
  if (tid == 0) {
    s_ij[0] = n;
    if constexpr (FIT) s_ij[1] = s_end[0];
    else s_ij[1] = m;
  }
  int n_match = 0, n_sub = 0, n_ins = 0, n_del = 0;  // thread 0's
  for (;;) {
    __syncthreads();
    const int ihi = s_ij[0], jhi = s_ij[1];
    if (ihi <= 0 || jhi <= 0) break;
    const int bhi = (jhi - 1) >> 4;
    {
      const int row = ihi - (tid >> 2), blk = bhi - (tid & 3);
      swin[tid >> 2][tid & 3] = row >= 1 && blk >= 0 ? aln_dir_word(full, rem, rem_bytes, W, r, row, blk) : 0u;
    }
    __syncthreads();
    if (tid == 0) {
      const int ilo = max(1, ihi - (ALN_WIN_ROWS - 1)), jlo = max(0, bhi - (ALN_WIN_BLKS - 1)) * 16 + 1;
      int i = ihi, j = jhi;
      while (i >= ilo && j >= jlo) {
        const int c = j - 1;
        const unsigned d = (swin[ihi - i][bhi - (c >> 4)] >> (2 * (c & 15))) & 3u;
        if (d == 0u) {
          const int sub = sa[i - 1] != sb[j - 1];
          n_sub += sub;
          n_match += 1 - sub;
          if (op) op[i - 1] = (unsigned char)sub;
          if constexpr (POS) rp[i - 1] = ob + j - 1;  // the reference base it is matched or mismatched to
          --i;
          --j;
        } else if (d == 1u) {
          ++n_ins;
          if (op) op[i - 1] = 2;
          if constexpr (POS) rp[i - 1] = ob + j - 1;  // the reference base to its left
          --i;
        } else {
          ++n_del;
          --j;
        }
      }
      s_ij[0] = i;
      s_ij[1] = j;
    }
  }
  const int ri = s_ij[0], rj = s_ij[1];  // a border: the rest of column 0 is insertions, the rest of row 0 deletions
  if (op)
    for (int x = tid; x < ri; x += ALN_THREADS) op[x] = 2;
  if constexpr (POS)
    for (int x = tid; x < ri; x += ALN_THREADS) rp[x] = ob - 1;
  if (tid == 0) {
    n_ins += max(ri, 0);
    if constexpr (FIT) {  // row 0 consumes nothing: the path starts at column rj of the window
      span[(size_t)p * 2] = ob + max(rj, 0);
      span[(size_t)p * 2 + 1] = ob + s_end[0];
    } else {
      n_del += max(rj, 0);
    }
    int* c = counts + (size_t)p * 5;
    c[0] = n_sub + n_ins + n_del;
    c[1] = n_match;
    c[2] = n_sub;
    c[3] = n_ins;
    c[4] = n_del;
  }
}

long long align_work_bytes(int P, long long cells) { return cells / 4 + 16ll * P + 64; }

hipError_t launch_align_seqs(const unsigned char* call, const int* call_off, const unsigned char* truth,
                             const int* truth_off, int P, long long cells, int* counts, unsigned char* ops,
                             int* status, void* work, hipStream_t s) {
  if (P < 0 || cells < 0 || cells > ALIGN_MAX_CELLS || !call_off || !truth_off ||
      (P > 0 && (!call || !truth || !counts || !status || !work)))
    return hipErrorInvalidValue;
  if (P == 0) return hipSuccess;
  long long* off = static_cast<long long*>(work);
  const long long head = 8ll * (P + 1);  // the offsets; the directions follow
  hipLaunchKernelGGL(align_offsets_kernel<false>, dim3(1), dim3(ALN_THREADS), 0, s, call_off, truth_off, P, off,
                     (const int*)nullptr, 0);
  hipLaunchKernelGGL((align_kernel<false, false>), dim3(P), dim3(ALN_THREADS), 0, s, call, call_off, truth, truth_off,
                     off, align_work_bytes(P, cells) - head, static_cast<unsigned char*>(work) + head, counts, ops,
                     status, (int*)nullptr, 0, (int*)nullptr);
  return hipGetLastError();
}

// rpos == nullptr: nd_align_fit, the instantiation without positions
hipError_t launch_align_fit(const unsigned char* call, const int* call_off, const unsigned char* ref, int ref_len,
                            const int* hit, int P, long long cells, int* counts, int* span, unsigned char* ops,
                            int* status, int* rpos, void* work, hipStream_t s) {
  if (P < 0 || cells < 0 || cells > ALIGN_MAX_CELLS || ref_len < 0 || !call_off ||
      (P > 0 && (!call || !ref || !hit || !counts || !span || !status || !work)))
    return hipErrorInvalidValue;
  if (P == 0) return hipSuccess;
  long long* off = static_cast<long long*>(work);
  const long long head = 8ll * (P + 1);
  hipLaunchKernelGGL(align_offsets_kernel<true>, dim3(1), dim3(ALN_THREADS), 0, s, call_off, hit, P, off,
                     (const int*)status, ref_len);
  const long long capacity = align_work_bytes(P, cells) - head;
  unsigned char* dirs = static_cast<unsigned char*>(work) + head;
  if (rpos)
    hipLaunchKernelGGL((align_kernel<true, true>), dim3(P), dim3(ALN_THREADS), 0, s, call, call_off, ref, hit, off,
                       capacity, dirs, counts, ops, status, span, ref_len, rpos);
  else
    hipLaunchKernelGGL((align_kernel<true, false>), dim3(P), dim3(ALN_THREADS), 0, s, call, call_off, ref, hit, off,
                       capacity, dirs, counts, ops, status, span, ref_len, (int*)nullptr);
  return hipGetLastError();
}

}  // namespace nd
