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
#include "common.hpp"
#include "kernels.hpp"

namespace nd {

#define ASM_THREADS 256
#define ASM_MAXLEN 199  // longest chunk assembled here (difflib autojunk starts at 200)

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

// one wave per chunk: its chars vote at pos[c] + x of the read's columns
__global__ void __launch_bounds__(ASM_THREADS)
asm_vote_kernel(const unsigned char* __restrict__ bases, const int* __restrict__ chunk_off,
                const int* __restrict__ read_off, const int* __restrict__ pos, const int* __restrict__ rd,
                const int* __restrict__ status, int C, int total, int* __restrict__ count) {
  const int c = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const int r = rd[c];
  if (status[r] != 0) return;
  const int o = chunk_off[c], len = chunk_off[c + 1] - o, p = pos[c];
  const int r0 = chunk_off[read_off[r]], cols = chunk_off[read_off[r + 1]] - r0;
  for (int x = lane; x < len; x += 64) {
    const int col = p + x, cls = asm_class(bases[o + x]);
    if (col >= 0 && col < cols && r0 + col < total && cls >= 0) atomicAdd(&count[(size_t)cls * total + r0 + col], 1);
  }
}

// one wave per chunk's span of the output: column g - r0 of read rd[c], 0 past the read's length
__global__ void __launch_bounds__(ASM_THREADS)
asm_call_kernel(const int* __restrict__ chunk_off, const int* __restrict__ read_off, const int* __restrict__ rd,
                const int* __restrict__ seq_len, const int* __restrict__ count, int C, int total,
                unsigned char* __restrict__ seq) {
  const int c = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const int r = rd[c];
  const int o = chunk_off[c], len = chunk_off[c + 1] - o;
  const int r0 = chunk_off[read_off[r]], n = seq_len[r];
  for (int x = lane; x < len; x += 64) {
    const int g = o + x;
    if (g >= total) break;
    unsigned char out = 0;
    if (g - r0 < n) {
      int best = count[g], cls = 0;
      for (int k = 1; k < 5; ++k) {
        const int v = count[(size_t)k * total + g];
        if (v > best) {
          best = v;
          cls = k;
        }
      }
      out = (unsigned char)((0x4D54474341ull >> (8 * cls)) & 0xFFu);  // "ACGTM"[cls]
    }
    seq[g] = out;
  }
}

size_t assemble_work_bytes(int C, long long total) {
  return (size_t)2 * C * sizeof(int) + (size_t)5 * total * sizeof(int);
}

hipError_t launch_assemble_reads(const unsigned char* bases, const int* chunk_off, const int* read_off, int R, int C,
                                 int total, unsigned char* seq, int* seq_len, int* status, void* work,
                                 hipStream_t s) {
  if (R < 0 || C < 0 || total < 0 || !chunk_off || !read_off || (R > 0 && (!seq_len || !status)) ||
      (C > 0 && !work) || (total > 0 && (!bases || !seq)))
    return hipErrorInvalidValue;
  if (R == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)R * sizeof(int), s);
  if (e != hipSuccess) return e;
  if (C == 0) return hipMemsetAsync(seq_len, 0, (size_t)R * sizeof(int), s);  // no chunks: every read is ""
  int* pos = static_cast<int*>(work);
  int* rd = pos + C;
  int* count = rd + C;
  if (total > 0) {
    e = hipMemsetAsync(count, 0, (size_t)5 * total * sizeof(int), s);
    if (e != hipSuccess) return e;
  }
  const int per = ASM_THREADS / 64;
  hipLaunchKernelGGL(asm_overlap_kernel, dim3(C), dim3(ASM_THREADS), 0, s, bases, chunk_off, read_off, R, pos, rd,
                     status);
  hipLaunchKernelGGL(asm_place_kernel, dim3(R), dim3(ASM_THREADS), 0, s, chunk_off, read_off, pos, status, seq_len);
  if (total > 0) {
    hipLaunchKernelGGL(asm_vote_kernel, dim3((C + per - 1) / per), dim3(ASM_THREADS), 0, s, bases, chunk_off,
                       read_off, pos, rd, status, C, total, count);
    hipLaunchKernelGGL(asm_call_kernel, dim3((C + per - 1) / per), dim3(ASM_THREADS), 0, s, chunk_off, read_off, rd,
                       seq_len, count, C, total, seq);
  }
  return hipGetLastError();
}

}  // namespace nd
