// Where a segment of a called read lies in a shared reference, and on which strand (nd_locate_segs): k-mer votes
// per diagonal bin, exactly the host rule of nanodecoder_amd/accuracy.py (locate_host).  The reference maps its
// reads outside its own code (pipeline.evaluate.sh: minimap2); there is no reference equivalent of this file.
//
// The rule.  Base codes A, C, G, T = 0..3, any other byte invalid.  A k-mer is MAP_K = 15 consecutive valid bases,
// its code the 30-bit number with the first base in the highest bits.  The index holds (code, pos) of every k-mer
// of the forward reference (inside one record, codes occurring more than MAP_OCC_MAX times removed), sorted by
// code, then pos.  For a segment q of n bases, strand 0 (q) and then strand 1 (its reverse complement, invalid
// bytes staying as they are):
//   every k-mer of the query at offset x and every index entry (code, y) with its code votes for bin
//   (y - x + MAP_SEG) >> MAP_BIN_SHIFT;  score[b] = votes[b] + votes[b + 1];
//   the hit is the (strand, b) of the largest score: strand 0 before strand 1, then the lowest b;
//   votes = that score; below MAP_MIN_VOTES, or n < MAP_K, or n > MAP_SEG: unmapped (status bit 0, window 0, 0).
// The window of a hit: lo = (b << 9) - MAP_SEG; its record the one containing clamp(lo + 512 + n div 2, 0,
// total - 1); w0 = max(record start, lo - MAP_PAD), w1 = min(record end, lo + 1024 + n + MAP_PAD).
//
// One workgroup of 256 threads per segment.  The oriented segment is in LDS as codes; a thread takes the offsets
// x = tid, tid + 256, ..., builds the k-mer, binary-searches the sorted codes (global memory: the same few
// megabytes for every workgroup, served by L2 / Infinity Cache) and adds one vote per entry to an LDS histogram
// of 16-bit counts, two bins to a 32-bit word: a bin holds at most (4096 - 14) * 8 = 32,656 votes, so the low
// half never carries into the high one.  Votes are integers: their order does not matter.  The bins are then
// scanned by all threads, each keeping its best (score, strand, b) as one 64-bit key, and the keys reduced in
// LDS.  Thread 0 derives the window; all threads write the oriented bytes.
//
// LDS: 32,788 (bins) + 4,112 (codes) + 2,048 (keys) = 38,948 bytes, 38,960 static with the arrays' alignment.
#include "common.hpp"
#include "kernels.hpp"

namespace nd {

#define LOC_THREADS 256
#define LOC_BINS (((MAP_REF_MAX + MAP_SEG) >> MAP_BIN_SHIFT) + 2)  // the last bin that can get a vote, + 1, + 1
#define LOC_WORDS ((LOC_BINS + 1) / 2)

__device__ __forceinline__ unsigned loc_code(unsigned char c) {
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 255u;
}
__device__ __forceinline__ unsigned char loc_complement(unsigned char c) {
  return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
}

__global__ void __launch_bounds__(LOC_THREADS)
locate_kernel(const unsigned char* __restrict__ call, const int* __restrict__ call_off,
              const unsigned* __restrict__ idx_code, const unsigned* __restrict__ idx_pos, int idx_len,
              const int* __restrict__ rec_off, int R, int* __restrict__ hit, int* __restrict__ status,
              unsigned char* __restrict__ call_or) {
  __shared__ unsigned sbin[LOC_WORDS];
  __shared__ __align__(16) unsigned char sq[MAP_SEG + 16];
  __shared__ unsigned long long skey[LOC_THREADS];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int oa = call_off[p], n = call_off[p + 1] - oa;
  const int total = rec_off[R];
  const bool can = n >= MAP_K && n <= MAP_SEG && total >= MAP_K && total <= MAP_REF_MAX && idx_len > 0;
  // bins 0 .. nbins - 1 can get a vote; bin nbins stays 0 for the last score
  const int nbins = can ? ((total + MAP_SEG) >> MAP_BIN_SHIFT) + 1 : 0;
  const int nwords = (nbins + 2) / 2;
  unsigned long long best = 0xFFFFFFFFull;  // score 0, strand 0, bin 0
  if (can) {
    for (int strand = 0; strand < 2; ++strand) {
      for (int x = tid; x < nwords; x += LOC_THREADS) sbin[x] = 0u;
      for (int x = tid; x < n + MAP_K; x += LOC_THREADS) {
        unsigned c = 255u;
        if (x < n) c = strand ? loc_code(loc_complement(call[oa + n - 1 - x])) : loc_code(call[oa + x]);
        sq[x] = (unsigned char)c;
      }
      __syncthreads();
      for (int x = tid; x + MAP_K <= n; x += LOC_THREADS) {
        unsigned code = 0u, any = 0u;
#pragma unroll
        for (int k = 0; k < MAP_K; ++k) {
          const unsigned c = sq[x + k];
          any |= c;
          code = (code << 2) | (c & 3u);
        }
        if (any > 3u) continue;  // an invalid base inside
        int lo = 0, hi = idx_len;  // the first entry with idx_code >= code
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (idx_code[mid] < code) lo = mid + 1;
          else hi = mid;
        }
        for (int e = lo; e < idx_len && e < lo + MAP_OCC_MAX && idx_code[e] == code; ++e) {
          const int bin = ((int)idx_pos[e] - x + MAP_SEG) >> MAP_BIN_SHIFT;
          if (bin >= 0 && bin < nbins) atomicAdd(&sbin[bin >> 1], 1u << (16 * (bin & 1)));
        }
      }
      __syncthreads();
      for (int b = tid; b < nbins; b += LOC_THREADS) {
        const unsigned w0 = sbin[b >> 1], w1 = sbin[(b + 1) >> 1];
        const unsigned score = ((w0 >> (16 * (b & 1))) & 0xFFFFu) + ((w1 >> (16 * ((b + 1) & 1))) & 0xFFFFu);
        // the largest key: the largest score, then strand 0, then the lowest bin
        const unsigned long long key = ((unsigned long long)score << 32) |
                                       (0xFFFFFFFFu - (((unsigned)strand << 24) | (unsigned)b));
        if (key > best) best = key;
      }
      __syncthreads();  // the bins are cleared next
    }
  }
  skey[tid] = best;
  __syncthreads();
  for (int o = LOC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o && skey[tid + o] > skey[tid]) skey[tid] = skey[tid + o];
    __syncthreads();
  }
  const unsigned long long win = skey[0];
  const int votes = (int)(win >> 32);
  const unsigned sb = 0xFFFFFFFFu - (unsigned)(win & 0xFFFFFFFFull);
  const int strand = (int)(sb >> 24), b = (int)(sb & 0xFFFFFFu);
  const bool mapped = can && votes >= MAP_MIN_VOTES;
  if (tid == 0) {
    int w0 = 0, w1 = 0;
    if (mapped) {
      const int lo = (b << MAP_BIN_SHIFT) - MAP_SEG;
      const int c = min(max(lo + (1 << MAP_BIN_SHIFT) + n / 2, 0), total - 1);
      int r0 = 0, r1 = R;  // the last record with rec_off[r] <= c
      while (r1 - r0 > 1) {
        const int mid = (r0 + r1) >> 1;
        if (rec_off[mid] <= c) r0 = mid;
        else r1 = mid;
      }
      w0 = max(rec_off[r0], lo - MAP_PAD);
      w1 = min(rec_off[r0 + 1], lo + (2 << MAP_BIN_SHIFT) + n + MAP_PAD);
    }
    int* h = hit + 4 * (size_t)p;
    h[0] = strand;
    h[1] = w0;
    h[2] = w1;
    h[3] = votes;
    status[p] = mapped ? 0 : 1;
  }
  if (strand) {
    for (int x = tid; x < n; x += LOC_THREADS) call_or[oa + x] = loc_complement(call[oa + n - 1 - x]);
  } else {
    for (int x = tid; x < n; x += LOC_THREADS) call_or[oa + x] = call[oa + x];
  }
}

hipError_t launch_locate_segs(const unsigned char* call, const int* call_off, int P, const unsigned* idx_code,
                              const unsigned* idx_pos, int idx_len, const int* rec_off, int R, int* hit, int* status,
                              unsigned char* call_or, hipStream_t s) {
  if (P < 0 || idx_len < 0 || R < 0 || !call_off || !rec_off || (idx_len > 0 && (!idx_code || !idx_pos)) ||
      (P > 0 && (!call || !hit || !status || !call_or)))
    return hipErrorInvalidValue;
  if (P == 0) return hipSuccess;
  hipLaunchKernelGGL(locate_kernel, dim3(P), dim3(LOC_THREADS), 0, s, call, call_off, idx_code, idx_pos, idx_len,
                     rec_off, R, hit, status, call_or);
  return hipGetLastError();
}

}  // namespace nd
