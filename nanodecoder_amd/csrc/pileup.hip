// Consensus of the mapped reads on the device (nd_pileup_add, nd_pileup_call): the pile of every oriented call base
// on the reference position nd_align_fit_pos gave it, and the call of a consensus base per position; exactly the
// host rule of nanodecoder_amd/accuracy.py (pile_add_host, consensus_host).  The reference evaluates its consensus
// outside its own code (scripts/analysis.sh: an assembler and a polisher); there is no reference equivalent of this
// file.
//
// The pile.  pile [9, ref_len] u32, plane by plane: A, C, G, T, D (deleted), iA, iC, iG, iT (an insertion after the
// position).  A base whose op is 0 or 1 is a diagonal base.  Every pair with status 0 adds
//   diagonal base i            : +1 in the plane of its code at rpos[i] (a byte other than A, C, G, T adds nothing);
//   with k the diagonal base of the pair before i, found by stepping back over the bases of op 2:
//     deleted positions        : +1 in D at every position strictly between rpos[k] and rpos[i];
//     an insertion run k+1..i-1: +1 in the i plane of the code of base k + 1, at rpos[k] (a run is one event, named
//                                by its first base);
//   leading and trailing insertions have no diagonal base on one side and add nothing.
// A position outside [0, ref_len) is skipped wherever it would add: rpos is not trusted.
//
// nd_pileup_add: one launch, a grid-stride loop with one thread per oriented call base of the whole batch; the
// pair of a base is a binary search in call_off.  Consecutive lanes hold consecutive bases, and the oriented call is
// on the forward strand, so a wave's 64 adds go to consecutive addresses (64 x 4 = 256 bytes, less the insertions
// and deletions in between) of at most four planes: the shape the chip's atomic units take at their full rate,
// where a row-major [ref_len, 9] table would put every add of the wave on a row of its own.  Unsigned integer
// atomics: the sums do not depend on the order of anything.
//
// The call.  At position r, cov = A + C + G + T + D (64-bit); cov < min_cov: cons = 255 and ins = 255; otherwise
// cons = the index 0..4 of the largest of the five counts, the lowest on a tie, and ins = the index of the largest
// of the four i counts (the lowest on a tie) when 2 (iA + iC + iG + iT) > cov, else 255.  Per record six 64-bit
// sums over its positions {called, match, sub, del, ins, cov_sum}: match = cons is the reference base's code, sub =
// cons < 4 and is not (a reference byte other than A, C, G, T counts here), del = cons == 4, ins = the called
// insertions, cov_sum over the called positions.
//
// nd_pileup_call: a memset of rec and one launch; a workgroup of 256 threads takes a stretch of 1024 consecutive
// positions, thread t the positions t, t + 256, ... of it (coalesced in all nine planes).  The records a stretch
// touches are consecutive; they are summed in LDS, PILE_RECS records at a time, and each non-zero sum leaves the
// workgroup as one 64-bit atomic.
#include "common.hpp"
#include "kernels.hpp"

namespace nd {

#define PILE_THREADS 256
#define PILE_ADD_GROUPS 2048  // the grid of the add kernel: 8 workgroups per CU, a grid-stride loop over the bases
#define PILE_PER_THREAD 4
#define PILE_STRETCH (PILE_THREADS * PILE_PER_THREAD)
#define PILE_RECS 32          // records summed in LDS at a time
#define PILE_PLANE_DEL 4
#define PILE_PLANE_INS 5

__device__ __forceinline__ int pile_code(unsigned char c) {
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 255;
}

// the largest p in [0, count) with off[p] <= x (0 when there is none); count >= 1
__device__ __forceinline__ int pile_slot(const int* __restrict__ off, int count, int x) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(PILE_THREADS)
pileup_add_kernel(const unsigned char* __restrict__ call, const int* __restrict__ call_off,
                  const unsigned char* __restrict__ ops, const int* __restrict__ rpos, const int* __restrict__ status,
                  int P, unsigned* __restrict__ pile, int ref_len) {
  const int total = call_off[P];
  const size_t plane = (size_t)ref_len;
  for (long long xx = (long long)blockIdx.x * PILE_THREADS + threadIdx.x; xx < total;
       xx += (long long)gridDim.x * PILE_THREADS) {
    const int x = (int)xx;
    if (ops[x] > 1) continue;  // an inserted base adds through the diagonal base after its run
    const int p = pile_slot(call_off, P, x);
    const int start = call_off[p];
    if (x < start || status[p] != 0) continue;
    const int r = rpos[x];
    const int code = pile_code(call[x]);
    if (code < 4 && r >= 0 && r < ref_len) atomicAdd(&pile[code * plane + r], 1u);
    int k = x - 1;
    while (k >= start && ops[k] == 2) --k;
    if (k < start || ops[k] > 1) continue;  // no diagonal base before this one: leading insertions are not piled
    const int rk = rpos[k];
    const long long q1 = min((long long)r, (long long)ref_len);
    for (long long q = max((long long)rk + 1, 0ll); q < q1; ++q) atomicAdd(&pile[PILE_PLANE_DEL * plane + q], 1u);
    if (k < x - 1) {
      const int first = pile_code(call[k + 1]);
      if (first < 4 && rk >= 0 && rk < ref_len) atomicAdd(&pile[(PILE_PLANE_INS + first) * plane + rk], 1u);
    }
  }
}

__global__ void __launch_bounds__(PILE_THREADS)
pileup_call_kernel(const unsigned* __restrict__ pile, const unsigned char* __restrict__ ref, int ref_len,
                   const int* __restrict__ rec_off, int R, int min_cov, unsigned char* __restrict__ cons,
                   unsigned char* __restrict__ ins, int* __restrict__ cov_out, unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long acc[PILE_RECS * 6];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * PILE_STRETCH;
  const size_t plane = (size_t)ref_len;
  int my_rec[PILE_PER_THREAD];                 // -1: nothing to add (past the end, uncalled, or in no record)
  unsigned my_kind[PILE_PER_THREAD];           // 1 match, 2 sub, 3 del; + 4 with a called insertion
  unsigned long long my_cov[PILE_PER_THREAD];
#pragma unroll
  for (int k = 0; k < PILE_PER_THREAD; ++k) {
    const long long pos = base + k * PILE_THREADS + tid;
    my_rec[k] = -1;
    my_kind[k] = 0;
    my_cov[k] = 0;
    if (pos >= ref_len) continue;
    unsigned c[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) c[q] = pile[q * plane + pos];
    const unsigned long long cov = (unsigned long long)c[0] + c[1] + c[2] + c[3] + c[4];
    cov_out[pos] = (int)cov;
    if (cov < (unsigned long long)min_cov) {
      cons[pos] = 255;
      ins[pos] = 255;
      continue;
    }
    int best = 0;
#pragma unroll
    for (int q = 1; q < 5; ++q)
      if (c[q] > c[best]) best = q;
    int ibest = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (c[PILE_PLANE_INS + q] > c[PILE_PLANE_INS + ibest]) ibest = q;
    const unsigned long long isum = (unsigned long long)c[5] + c[6] + c[7] + c[8];
    const bool has_ins = 2 * isum > cov;
    cons[pos] = (unsigned char)best;
    ins[pos] = has_ins ? (unsigned char)ibest : (unsigned char)255;
    const int rr = pile_slot(rec_off, R, (int)pos);
    if (pos < rec_off[rr] || pos >= rec_off[rr + 1]) continue;
    my_rec[k] = rr;
    my_kind[k] = (best == 4 ? 3u : best == pile_code(ref[pos]) ? 1u : 2u) | (has_ins ? 4u : 0u);
    my_cov[k] = cov;
  }
  // the records of the stretch are consecutive: from that of its first position to that of its last
  const int r0 = pile_slot(rec_off, R, (int)base);
  const int r1 = pile_slot(rec_off, R, (int)min(base + PILE_STRETCH - 1, (long long)ref_len - 1));
  for (int c0 = r0; c0 <= r1; c0 += PILE_RECS) {
    if (tid < PILE_RECS * 6) acc[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PILE_PER_THREAD; ++k) {
      const int rel = my_rec[k] - c0;
      if (my_rec[k] < 0 || rel < 0 || rel >= PILE_RECS) continue;
      unsigned long long* a = &acc[rel * 6];
      atomicAdd(&a[0], 1ull);
      atomicAdd(&a[my_kind[k] & 3u], 1ull);  // 1 match, 2 sub, 3 del
      if (my_kind[k] & 4u) atomicAdd(&a[4], 1ull);
      atomicAdd(&a[5], my_cov[k]);
    }
    __syncthreads();
    if (tid < PILE_RECS * 6 && c0 + tid / 6 <= r1) {
      const unsigned long long v = acc[tid];
      if (v) atomicAdd(&rec[(size_t)(c0 + tid / 6) * 6 + tid % 6], v);
    }
    __syncthreads();
  }
}

hipError_t launch_pileup_add(const unsigned char* call, const int* call_off, const unsigned char* ops, const int* rpos,
                             const int* status, int P, unsigned* pile, int ref_len, hipStream_t s) {
  if (P < 0 || ref_len < 0 || !call_off || (P > 0 && (!call || !ops || !rpos || !status || !pile)))
    return hipErrorInvalidValue;
  if (P == 0 || ref_len == 0) return hipSuccess;
  hipLaunchKernelGGL(pileup_add_kernel, dim3(PILE_ADD_GROUPS), dim3(PILE_THREADS), 0, s, call, call_off, ops, rpos,
                     status, P, pile, ref_len);
  return hipGetLastError();
}

hipError_t launch_pileup_call(const unsigned* pile, const unsigned char* ref, int ref_len, const int* rec_off, int R,
                              int min_cov, unsigned char* cons, unsigned char* ins, int* cov, long long* rec,
                              hipStream_t s) {
  if (ref_len < 0 || R < 0 || min_cov < 1) return hipErrorInvalidValue;
  if (R == 0 || ref_len == 0) return hipSuccess;
  if (!pile || !ref || !rec_off || !cons || !ins || !cov || !rec) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(rec, 0, (size_t)R * 6 * sizeof(long long), s);
  if (e != hipSuccess) return e;
  const unsigned groups = (unsigned)(((long long)ref_len + PILE_STRETCH - 1) / PILE_STRETCH);
  hipLaunchKernelGGL(pileup_call_kernel, dim3(groups), dim3(PILE_THREADS), 0, s, pile, ref, ref_len, rec_off, R,
                     min_cov, cons, ins, cov, reinterpret_cast<unsigned long long*>(rec));
  return hipGetLastError();
}

}  // namespace nd
