// gpu_check — an active device check with exact answers: "is this GPU bad, or was it the job?"
//
//   gpu_check gemm [--dtype bf16|mxfp8|mxfp4|fp64|int8] --m M --n N --k K [--seed S]
//                  [--a FILE --b FILE [--sa FILE --sb FILE]] [--c-out FILE]
//                  [--poison I,J] [--device D] [--seconds T]
//        bf16 x bf16 -> fp32 GEMM on the matrix units (v_mfma_f32_32x32x16_bf16), checked on
//        the device by Huang-Abraham checksums.  Every element of A (M x K, row-major) and
//        B (N x K, K-contiguous) is an integer in [-2, 2], so every product, partial sum and
//        checksum is an integer of magnitude <= 4*K*128 <= 2^24 and fp32 holds it exactly in
//        any summation order: a healthy device agrees bit for bit with integer arithmetic and
//        the comparison is ==, no tolerance.  The expected checksums come from integer kernels
//        that share nothing with the matrix path.
//        --dtype mxfp8 / mxfp4: the same check in the OCP microscaling formats on the scaled
//        matrix path (v_mfma_scale_f32_32x32x64_f8f6f4): E4M3 or E2M1 elements with one E8M0
//        scale per 32 consecutive k, SA[M][K/32] and SB[N][K/32], each 127 or 128 (x1 or x2)
//        and varying per (row, block).
//          mxfp8: elements are integers in [-2, 2] (bytes 00 38 40 B8 C0), so a scaled product
//          is an integer of magnitude <= (2*2)*(2*2) = 16 and a checksum over 128 rows of K
//          products is at most 16*K*128 <= 2^24 for K <= 8192.
//          mxfp4: elements are in {0, +-0.5, +-1, +-1.5, +-2} (codes 0..4, sign in bit 3; two
//          per byte, even k in the low nibble), so a scaled product is a multiple of 1/4 of
//          magnitude <= 16 = 64 quarter-units and 64*K*128 <= 2^24 for K <= 2048.
//        Within those caps fp32 is again exact in any order and the comparison stays ==; the
//        expected checksums are integers in units of 1 (mxfp8) or 1/4 (mxfp4).  --a/--b are
//        raw element bytes (M*K, N*K; for mxfp4 half that), --sa/--sb the scale bytes.
//        --dtype fp64: the same check on the double-precision matrix path
//        (v_mfma_f64_16x16x4_f64), which none of the above touches, and on wide data.  A and B
//        are little-endian IEEE doubles, every element an integer of magnitude <= 65535, roughly
//        uniform over that range when generated: not five-valued.  A product is below 2^32 and a
//        checksum over 128 rows of K products below 2^32 * K * 128 <= 2^52 for K <= 8192, so
//        every partial sum in any order is an integer below 2^53, FP64 holds it exactly and the
//        comparison stays ==.  M and N are multiples of 16, K a multiple of 4 and at most 8192.
//        --a/--b hold M*K and N*K doubles (a negative zero is accepted), --c-out M*N doubles.
//        The expected checksums come from kernels that decode the doubles' bit patterns with
//        integer operations and add in int64: no instruction of the double-precision unit, a
//        conversion included, is on that side.
//        --dtype int8: the same check on the integer matrix path (v_mfma_i32_32x32x32_i8), on
//        full-range data.  A and B are raw int8 bytes, uniform over all 256 values (-128 among
//        them) when generated.  Integers need no exactness trick: |element| <= 128, so
//        |product| <= 2^14 and |C[i][j]| <= 2^14 * K <= 2^30 for K <= 65536, inside int32 whatever
//        the data (whether the accumulate wraps or saturates past that never arises).  A checksum
//        over 128 rows or columns is at most 2^37: the epilogue sums the int32 accumulators in
//        int64, and checksums and expectations are 8 bytes.  M and N are multiples of 32, K a
//        multiple of 32 and at most 65536.  --a/--b hold M*K and N*K bytes, every byte valid;
//        --c-out M*N int32.  The expected checksums are plain integer multiply-adds.
//   gpu_check hbm --mib SIZE [--passes P] [--seed S] [--flip WORD:MASK] [--device D]
//        moving inversions over one allocation: pass 0 writes an address hash, each later pass
//        loads, compares with what the pass before wrote and stores the next pattern (odd
//        passes store the bitwise complement, so every cell is held in both states); a last
//        read-only sweep checks what the final pass wrote.
//   gpu_check cu [--k K] [--reps R] [--passes P] [--rounds N] [--seed S]
//                [--flip WG:WORD:MASK] [--poison WG:WAVE:I,J] [--device D]
//        *where on the die*: one workgroup per compute unit, each holding the CU's whole 160 KB of
//        LDS so that no two share a CU.  Every wave reads the hardware-ID status registers, and
//        the workgroup reports per physical CU (XCC, SE, SH, CU) and SIMD.  It runs the moving
//        inversions of `hbm` over all 40960 words of the CU's LDS (--passes, default 4), then on
//        each of its 16 waves a chain of K / 16 v_mfma_f32_32x32x16_bf16 (--k, a multiple of 16,
//        at most and by default 304: what the operands of 16 waves take of the LDS) from zeroed
//        accumulators, --reps times (default 16), each compared with == against the same dot
//        products in 32-bit integer arithmetic on the same LDS operands: integers in [-2, 2], a
//        sum of magnitude <= 4 K, exact in fp32.  One launch is a round; the dispatcher may reuse
//        a CU that has just become free, so up to --rounds (default 8) are launched until every
//        CU and every SIMD of it has been seen.  A check that did not reach a CU has not cleared
//        it: incomplete coverage is exit 1 with "error":"coverage".  The verdict needs an
//        otherwise idle device.  --flip xors one LDS word of workgroup WG after the first write
//        pass, --poison adds 1 to element I,J of one wave's block after its first chain, both in
//        round 0 only.
//   gpu_check attn [--heads H] [--seq S] [--d 64|128] [--causal] [--seed S] [--seconds T]
//                  [--q FILE --k FILE --v FILE] [--o-out FILE] [--ml-out FILE]
//                  [--poison H,I,C] [--device D]
//        fused attention, the data flow none of the above has: matrix accumulators read back by
//        the vector ALU and fed to the matrix unit again as operands, register to register; row
//        reductions across lanes; the transcendental unit (v_exp_f32); the fp32 -> bf16 pack;
//        the per-row rescale of live accumulators (online softmax); with --causal the masked
//        diagonal tile.  Per head, with Q, K, V of shape S x d in bf16, row-major:
//          s[i][j] = sum_c Q[i][c] K[j][c]     (no 1/sqrt(d): it would add nothing to the check)
//          m[i] = max_j s[i][j],  p[i][j] = 2^(s[i][j] - m[i]),  l[i] = sum_j p[i][j]
//          O'[i][c] = sum_j p[i][j] V[j][c]    (unnormalised; with --causal j runs over j <= i)
//        The final division by l is not correctly rounded on the device, so it stays out:
//        v_rcp_f32 remains uncovered.  Both sides are exact and the comparison is ==:
//          K and V elements are integers in [-2, 2] (the five values of the GEMM inputs) and every
//          row of Q holds integers with sum_c |Q[i][c]| <= 3, so |s| <= 6 and s - m is an integer
//          in [-12, 0]: every p is a power of two no smaller than 2^-12, exact in bf16.
//          With online softmax the running maximum never exceeds the final one, so at every step
//          l and O' are integer multiples of 2^-12 with l <= S and |O'| <= 2 S; fp32 holds all of
//          them exactly, in any summation order, while 2 S 2^12 <= 2^24, that is S <= 2048.
//          The rescale factor 2^(m_old - m_new) is a power of two no smaller than 2^-12 and
//          keeps the unit; the fp32 -> bf16 conversion of a power of two is exact under any
//          rounding mode.
//        S is a multiple of 64 and at most 2048, d is 64 or 128, H from 1 to 65535 (the grid);
//        the defaults are 64 heads, S 2048, d 128, not causal, a pass of about a millisecond.
//        --q/--k/--v hold H*S*d bf16 each and every element is checked against the rules above
//        before the device is opened.  When generated, a row of Q has +-1 at three hashed
//        columns, summed where they collide.  The expected O', l and m come once per run from an
//        integer kernel (shifts, no floating-point instruction); the device's fp32 results are
//        decoded to units of 2^-12 by bit pattern and compared after every pass.  --o-out and
//        --ml-out dump O' (H x S x d fp32) and the pairs (m, l) (H x S x 2 fp32); --poison adds
//        2^-12 to O'[H][I][C].  A mismatch record is {"kind": "o" | "l" | "m", "head", "i", "c",
//        "delta"}: delta in units of 2^-12, c 0 for l and m; wrong O' elements first, then l and
//        m, each in index order.
//
// The last stdout line is one JSON object.  Exit 0: every check passed; 1: wrong data found;
// 2: usage error; 3: a HIP call failed.  --poison and --flip are the detectors' self-tests:
// they alter data only, never provoke a fault.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static const char* g_check = "gemm";

#define CHECK(x)                                                                             \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) {                                                                  \
      fprintf(stderr, "%s failed: %s (%s)\n", #x, hipGetErrorName(e_), hipGetErrorString(e_)); \
      printf("{\"check\":\"%s\",\"ok\":false,\"error\":\"%s: %s\"}\n", g_check, #x, hipGetErrorName(e_)); \
      exit(3);                                                                               \
    }                                                                                        \
  } while (0)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ static inline uint32_t mix32(uint32_t x) {  // a bijection on 32 bits
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// ------------------------------------------------------------------------------------------
// GEMM inputs: integers in [-2, 2] as bf16 bit patterns
// ------------------------------------------------------------------------------------------

__device__ static inline uint32_t small_int_bf16(uint32_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = mix32(mix32(seed ^ (row * 0x9e3779b9u)) + col);
  const int v = static_cast<int>(h % 5u) - 2;
  return v == 0 ? 0u : ((v < 0 ? 0x8000u : 0u) | ((v == 2 || v == -2) ? 0x4000u : 0x3f80u));
}

// X is rows x K; one thread writes 8 consecutive bf16 (16 bytes).  K is a multiple of 16.
__global__ __launch_bounds__(256) void generate_kernel(uint16_t* __restrict__ x, int rows, int K, uint32_t seed) {
  const size_t chunks = static_cast<size_t>(rows) * (K / 8);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t c = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; c < chunks; c += stride) {
    const uint32_t row = static_cast<uint32_t>(c / (K / 8)), col = static_cast<uint32_t>(c % (K / 8)) * 8;
    u32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      v[e] = small_int_bf16(seed, row, col + 2 * e) | (small_int_bf16(seed, row, col + 2 * e + 1) << 16);
    *reinterpret_cast<u32x4*>(x + c * 8) = v;
  }
}

// The microscaling inputs, from the same hash.  X is rows x K elements; one thread writes 16
// bytes: 16 E4M3 bytes, or 32 E2M1 nibbles (one whole scale block).  K is a multiple of 64.
enum Fmt { BF16 = 0, MXFP8 = 1, MXFP4 = 2, FP64 = 3, INT8 = 4 };

template <int FMT>
__device__ static inline uint32_t small_mx_code(uint32_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = mix32(mix32(seed ^ (row * 0x9e3779b9u)) + col);
  if (FMT == MXFP8) {  // -2 .. 2
    const int v = static_cast<int>(h % 5u) - 2;
    return v == 0 ? 0u : ((v < 0 ? 0x80u : 0u) | ((v == 2 || v == -2) ? 0x40u : 0x38u));
  }
  const int v = static_cast<int>(h % 9u) - 4;  // half-units -4 .. 4: the code is the magnitude
  return v < 0 ? 8u | static_cast<uint32_t>(-v) : static_cast<uint32_t>(v);
}

template <int FMT>
__global__ __launch_bounds__(256) void generate_mx_kernel(unsigned char* __restrict__ x, int rows, int K, uint32_t seed) {
  constexpr int PER = FMT == MXFP8 ? 16 : 32;  // elements per 16-byte chunk
  const size_t chunks = static_cast<size_t>(rows) * (K / PER);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t c = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; c < chunks; c += stride) {
    const uint32_t row = static_cast<uint32_t>(c / (K / PER)), col = static_cast<uint32_t>(c % (K / PER)) * PER;
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < PER; ++e)  // element e sits at bit e * (128 / PER) of the chunk
      v[e / (PER / 4)] |= small_mx_code<FMT>(seed, row, col + e) << (e % (PER / 4) * (128 / PER));
    *reinterpret_cast<u32x4*>(x + c * 16) = v;
  }
}

// S is rows x K/32 E8M0 bytes, each 127 or 128; salted so that it is no function of the elements
__global__ __launch_bounds__(256) void generate_scale_kernel(unsigned char* __restrict__ s, int rows, int KS, uint32_t seed) {
  const size_t n = static_cast<size_t>(rows) * KS;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t x = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; x < n; x += stride) {
    const uint32_t row = static_cast<uint32_t>(x / KS), blk = static_cast<uint32_t>(x % KS);
    s[x] = 127u + (mix32(mix32(~seed ^ (row * 0x9e3779b9u)) + blk) >> 31);
  }
}

// The FP64 inputs, from the same hash: integers roughly uniform over [-65535, 65535] as IEEE
// double bit patterns, put together with integer operations (the data is then the same whatever
// the double-precision unit does).  One thread writes 2 doubles (16 bytes); K is a multiple of 4.
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

__device__ static inline uint64_t wide_int_f64(uint32_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = mix32(mix32(seed ^ (row * 0x9e3779b9u)) + col);
  const int v = static_cast<int>(h % 131071u) - 65535;
  if (v == 0) return 0ull;
  const uint32_t mag = static_cast<uint32_t>(v < 0 ? -v : v);
  const int p = 31 - __clz(static_cast<int>(mag));  // mag = 2^p + rest
  return (static_cast<uint64_t>(v < 0) << 63) | (static_cast<uint64_t>(1023 + p) << 52) |
         (static_cast<uint64_t>(mag ^ (1u << p)) << (52 - p));
}

__global__ __launch_bounds__(256) void generate_f64_kernel(uint64_t* __restrict__ x, int rows, int K, uint32_t seed) {
  const size_t chunks = static_cast<size_t>(rows) * (K / 2);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t c = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; c < chunks; c += stride) {
    const uint32_t row = static_cast<uint32_t>(c / (K / 2)), col = static_cast<uint32_t>(c % (K / 2)) * 2;
    const u64x2 v = {wide_int_f64(seed, row, col), wide_int_f64(seed, row, col + 1)};
    *reinterpret_cast<u64x2*>(x + c * 2) = v;
  }
}

// The INT8 inputs, from the same hash: the low byte of it, so every one of the 256 values occurs,
// -128 included.  X is rows x K bytes; one thread writes 16 of them.  K is a multiple of 32.
__global__ __launch_bounds__(256) void generate_i8_kernel(unsigned char* __restrict__ x, int rows, int K, uint32_t seed) {
  const size_t chunks = static_cast<size_t>(rows) * (K / 16);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t c = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; c < chunks; c += stride) {
    const uint32_t row = static_cast<uint32_t>(c / (K / 16)), col = static_cast<uint32_t>(c % (K / 16)) * 16;
    const uint32_t hr = mix32(seed ^ (row * 0x9e3779b9u));
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e / 4] |= (mix32(hr + col + e) & 0xffu) << (e % 4 * 8);
    *reinterpret_cast<u32x4*>(x + c * 16) = v;
  }
}

// ------------------------------------------------------------------------------------------
// The GEMM with checksum epilogue
// ------------------------------------------------------------------------------------------

constexpr int TILE = 128;                  // C tile edge per workgroup
constexpr int KSTEP = 64;                  // K advance per LDS stage
constexpr int ROW_BYTES = KSTEP * 2 + 16;  // 128 B of data + 16 B pad
constexpr int STAGE_BYTES = TILE * ROW_BYTES;

// The checksum epilogue of both GEMM kernels, from registers: the 128x128 tile is held as 2x2
// blocks of 32x32 accumulators per wave, register r of lane l holding
// D[8 * (r / 4) + 4 * (l / 32) + r % 4][l % 32].  `red` is 512 floats of LDS that no wave reads
// any more.  Element (bm, bn, r) of this lane is
//   row  row0 + wm*64 + bm*32 + 8*(r/4) + 4*half + r%4,   column  col0 + wn*64 + bn*32 + l32.
__device__ __forceinline__ void abft_epilogue(f32x16 (&acc)[2][2], float* red, int M, int N, float* __restrict__ colsum,
                                              float* __restrict__ rowsum, float* __restrict__ C, int poison_i,
                                              int poison_j) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l32 = lane & 31, half = lane >> 5;
  const int tn = blockIdx.x, tm = blockIdx.y;
  const int row0 = tm * TILE, col0 = tn * TILE;
  const int lane_row = row0 + wm * 64 + 4 * half, lane_col = col0 + wn * 64 + l32;
  if (poison_i >= 0) {  // detector self-test: one element off by one
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool hit = lane_row + bm * 32 + 8 * (r >> 2) + (r & 3) == poison_i && lane_col + bn * 32 == poison_j;
          acc[bm][bn][r] += hit ? 1.0f : 0.0f;
        }
  }

  // red [0,256): column partials by wm; [256,512): row partials by wn
  // column sums: over this lane's 32 registers, then across the two half-waves
#pragma unroll
  for (int bn = 0; bn < 2; ++bn) {
    float cs = 0.0f;
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int r = 0; r < 16; ++r) cs += acc[bm][bn][r];
    cs += __shfl_xor(cs, 32);
    if (half == 0) red[wm * TILE + wn * 64 + bn * 32 + l32] = cs;
  }
  // row sums: per register over both column blocks, then a butterfly over the 32 lanes of a half-wave
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float rs = acc[bm][0][r] + acc[bm][1][r];
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) rs += __shfl_xor(rs, off);
      if (l32 == 0) red[2 * TILE + wn * TILE + wm * 64 + bm * 32 + 8 * (r >> 2) + 4 * half + (r & 3)] = rs;
    }
  __syncthreads();
  if (t < TILE) {
    if (col0 + t < N) colsum[static_cast<size_t>(tm) * N + col0 + t] = red[t] + red[TILE + t];
  } else {
    const int u = t - TILE;
    if (row0 + u < M) rowsum[static_cast<size_t>(tn) * M + row0 + u] = red[2 * TILE + u] + red[3 * TILE + u];
  }

  if (C != nullptr) {  // --c-out only; the production run never stores M x N
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = lane_row + bm * 32 + 8 * (r >> 2) + (r & 3), col = lane_col + bn * 32;
          if (row < M && col < N) C[static_cast<size_t>(row) * N + col] = acc[bm][bn][r];
        }
  }
}

// Compiled for gfx950 (-O3, kernel-resource-usage): 112 VGPRs + 64 AGPRs (the accumulators),
// 73728 B LDS, 0 scratch, 0 SGPR/VGPR spills; occupancy 2 waves per SIMD (two workgroups per
// CU, bounded by LDS: 2 x 72 KB of 160 KB).
//
// One workgroup (4 waves) owns a 128x128 tile of C; wave w owns the 64x64 quadrant
// (w / 2, w % 2) as 2x2 blocks of v_mfma_f32_32x32x16_bf16: 4 accumulators of 16 VGPRs.
//
// Operand layout of the instruction (CDNA4 ISA guide, matrix arithmetic): lane l supplies
// row (A) or column (B) l % 32 and the 8 consecutive k values 8 * (l / 32) .. + 7; accumulator
// register r of lane l holds D[8 * (r / 4) + 4 * (l / 32) + r % 4][l % 32].
//
// LDS: per stage a 128 x 64 bf16 tile of A and one of B, two stages.  Rows are *padded* from
// 128 to 144 bytes (chosen over an xor swizzle: the address is one multiply-add, and the
// global->LDS copy keeps whole 16-byte chunks).  An operand read is one ds_read_b128 per
// lane; the 16 lanes served together read rows r .. r+15 at one k offset, i.e. start banks
// 36 * r mod 64 = {0,36,8,44,16,52,24,60,32,4,40,12,48,20,56,28}: sixteen distinct
// 4-bank groups covering all 64 banks once, so the reads are conflict-free (with 32 banks
// and 8 lanes per pass it is 4 * r mod 32, equally distinct).  The stage writes (8 lanes
// per row) overlap by 4 banks at the row seam; they are a quarter of the LDS traffic.
//
// Rows past M, columns past N and k past K are zero-filled in LDS, never read from memory.
// K is a multiple of 16 and a row starts 16-byte aligned, so an 8-element chunk is wholly
// inside or wholly outside.
__global__ __launch_bounds__(256) void gemm_abft_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                        int M, int N, int K, float* __restrict__ colsum,
                                                        float* __restrict__ rowsum, float* __restrict__ C,
                                                        int poison_i, int poison_j) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * STAGE_BYTES];  // [stage][A, B]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l32 = lane & 31, half = lane >> 5;
  const int tn = blockIdx.x, tm = blockIdx.y;
  const int row0 = tm * TILE, col0 = tn * TILE;

  // global -> LDS copy: a stage tile is 1024 16-byte chunks, 4 per thread per operand;
  // 8 consecutive lanes cover one 128-byte row segment
  const int lr = t >> 3, kc = t & 7;
  u32x4 ga[4], gb[4];
  const u32x4 zero = {0u, 0u, 0u, 0u};

#define LOAD_GLOBAL(k0)                                                                        \
  do {                                                                                         \
    const int k_ = (k0) + kc * 8;                                                              \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
      const int ra_ = row0 + lr + 32 * q, rb_ = col0 + lr + 32 * q;                            \
      ga[q] = (ra_ < M && k_ < K) ? *reinterpret_cast<const u32x4*>(A + static_cast<size_t>(ra_) * K + k_) : zero; \
      gb[q] = (rb_ < N && k_ < K) ? *reinterpret_cast<const u32x4*>(B + static_cast<size_t>(rb_) * K + k_) : zero; \
    }                                                                                          \
  } while (0)
#define STORE_LDS(stage)                                                                       \
  do {                                                                                         \
    unsigned char* d_ = lds + (stage) * 2 * STAGE_BYTES + lr * ROW_BYTES + kc * 16;            \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
      *reinterpret_cast<u32x4*>(d_ + 32 * q * ROW_BYTES) = ga[q];                              \
      *reinterpret_cast<u32x4*>(d_ + STAGE_BYTES + 32 * q * ROW_BYTES) = gb[q];                \
    }                                                                                          \
  } while (0)

  f32x16 acc[2][2];
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int bn = 0; bn < 2; ++bn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bm][bn][r] = 0.0f;

  const int nsteps = (K + KSTEP - 1) / KSTEP;
  LOAD_GLOBAL(0);
  STORE_LDS(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int stage = s & 1;
    const bool more = s + 1 < nsteps;
    if (more) LOAD_GLOBAL((s + 1) * KSTEP);  // in flight while this step multiplies
    const unsigned char* sa = lds + stage * 2 * STAGE_BYTES + (wm * 64 + l32) * ROW_BYTES + half * 16;
    const unsigned char* sb = lds + stage * 2 * STAGE_BYTES + STAGE_BYTES + (wn * 64 + l32) * ROW_BYTES + half * 16;
#pragma unroll
    for (int kk = 0; kk < KSTEP / 16; ++kk) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(sa + kk * 32);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(sa + 32 * ROW_BYTES + kk * 32);
      const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(sb + kk * 32);
      const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(sb + 32 * ROW_BYTES + kk * 32);
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
    }
    // the other stage was last read in step s-1, before the barrier that ended it
    if (more) STORE_LDS(stage ^ 1);
    __syncthreads();
  }
#undef LOAD_GLOBAL
#undef STORE_LDS

  abft_epilogue(acc, reinterpret_cast<float*>(lds), M, N, colsum, rowsum, C, poison_i, poison_j);
}

// ------------------------------------------------------------------------------------------
// The microscaling GEMM (MXFP8, MXFP4) with the same checksum epilogue
// ------------------------------------------------------------------------------------------

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MX_ROW_BYTES = 128;  // one stage row: 128 k of fp8 or 256 k of fp4, no padding
constexpr int MX_STAGE_BYTES = TILE * MX_ROW_BYTES;

// Four consecutive E8M0 bytes of one row of S (rows x KS) from block kb, a multiple of 4; 127
// (x1.0) where there is no row or no block: those elements are zero-filled anyway.  K is a
// multiple of 64, so KS is even: a row starts 2-byte aligned (4-byte when K is a multiple of
// 128) and ends on a whole or a half word, and nothing outside the row is read.
__device__ static inline uint32_t load_scale_word(const unsigned char* __restrict__ S, int row, int rows, int KS, int kb) {
  uint32_t w = 0x7f7f7f7fu;
  if (row < rows && kb < KS) {
    const void* p = __builtin_assume_aligned(S + static_cast<size_t>(row) * KS + kb, 2);
    if (kb + 4 <= KS) {
      __builtin_memcpy(&w, p, 4);
    } else {
      uint16_t h;
      __builtin_memcpy(&h, p, 2);
      w = 0x7f7f0000u | h;
    }
  }
  return w;
}

// The 64 k of one instruction for this wave's 2x2 blocks.  `pa`/`pb` are the lane's LDS rows,
// `ch` its (swizzled) first 16-byte chunk; the scale words were shifted by 8 * half when loaded, so
// that OPSEL (an immediate: byte 0 or 2) serves both half-waves.
template <int FMT, int OPSEL>
__device__ __forceinline__ void mx_mfma_2x2(const unsigned char* pa, const unsigned char* pb, int ch, uint32_t sa0,
                                            uint32_t sa1, uint32_t sb0, uint32_t sb1, f32x16 (&acc)[2][2]) {
  constexpr int CB = FMT == MXFP4 ? 4 : 0;  // cbsz / blgp: E4M3 or E2M1
  const i32x4 a0l = *reinterpret_cast<const i32x4*>(pa + ch * 16);
  const i32x4 a1l = *reinterpret_cast<const i32x4*>(pa + 32 * MX_ROW_BYTES + ch * 16);
  const i32x4 b0l = *reinterpret_cast<const i32x4*>(pb + ch * 16);
  const i32x4 b1l = *reinterpret_cast<const i32x4*>(pb + 32 * MX_ROW_BYTES + ch * 16);
  i32x8 a0, a1, b0, b1;
  if (FMT == MXFP8) {  // 32 bytes per lane: this chunk of the first block and the same of the second
    const int c2 = (ch ^ 2) * 16;
    a0 = __builtin_shufflevector(a0l, *reinterpret_cast<const i32x4*>(pa + c2), 0, 1, 2, 3, 4, 5, 6, 7);
    a1 = __builtin_shufflevector(a1l, *reinterpret_cast<const i32x4*>(pa + 32 * MX_ROW_BYTES + c2), 0, 1, 2, 3, 4, 5, 6, 7);
    b0 = __builtin_shufflevector(b0l, *reinterpret_cast<const i32x4*>(pb + c2), 0, 1, 2, 3, 4, 5, 6, 7);
    b1 = __builtin_shufflevector(b1l, *reinterpret_cast<const i32x4*>(pb + 32 * MX_ROW_BYTES + c2), 0, 1, 2, 3, 4, 5, 6, 7);
  } else {  // 16 bytes per lane; with cbsz/blgp 4 the upper four registers are not read
    a0 = __builtin_shufflevector(a0l, a0l, 0, 1, 2, 3, -1, -1, -1, -1);
    a1 = __builtin_shufflevector(a1l, a1l, 0, 1, 2, 3, -1, -1, -1, -1);
    b0 = __builtin_shufflevector(b0l, b0l, 0, 1, 2, 3, -1, -1, -1, -1);
    b1 = __builtin_shufflevector(b1l, b1l, 0, 1, 2, 3, -1, -1, -1, -1);
  }
  acc[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b0, acc[0][0], CB, CB, OPSEL, sa0, OPSEL, sb0);
  acc[0][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b1, acc[0][1], CB, CB, OPSEL, sa0, OPSEL, sb1);
  acc[1][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b0, acc[1][0], CB, CB, OPSEL, sa1, OPSEL, sb0);
  acc[1][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b1, acc[1][1], CB, CB, OPSEL, sa1, OPSEL, sb1);
}

// Compiled for gfx950 (-O3, kernel-resource-usage):
//   MXFP8: 152 VGPRs + 64 AGPRs (the accumulators), 65536 B LDS, 0 scratch, 0 SGPR/VGPR spills
//   MXFP4: 162 VGPRs + 64 AGPRs, 65536 B LDS, 0 scratch, 0 SGPR/VGPR spills
// both at occupancy 2 waves per SIMD: two workgroups per CU, bounded by LDS (2 x 64 KB of
// 160 KB) and equally by registers (216 and 226 of 512 per SIMD lane).
//
// The work split is that of gemm_abft_kernel: one workgroup (4 waves) per 128x128 tile of C,
// wave w the 64x64 quadrant (w / 2, w % 2) as 2x2 blocks, here of
// v_mfma_scale_f32_32x32x64_f8f6f4; the epilogue is shared.  What differs is how the data moves.
//
// Operand layout of the instruction (CDNA4 ISA guide, matrix arithmetic; settled on the device
// by the one-instruction shape of the tests): lane l supplies row (A) or column (B) l % 32, and
// its scale register (one E8M0 byte of it, picked by OPSEL: the immediate is the byte index)
// scales the MX block l / 32 of the 64 k, for every lane of that row.
//   E2M1 (cbsz/blgp 4): four registers, the 32 consecutive k of block l / 32, lower k in the low
//   nibble: one MX block is exactly one lane's operand.
//   E4M3: eight registers, but *not* 32 consecutive k: registers 0..3 are the 16 k from
//   16 * (l / 32) of block 0 and registers 4..7 the 16 k from 16 * (l / 32) of block 1.  Each
//   half-wave holds half of both blocks, and a lane's scale also applies to the other
//   half-wave's registers of that block.  (Fed as 32 consecutive k per lane the products are
//   right and the scales are crossed: all-ones elements or all-equal scales do not show it.)
// The accumulator layout is that of the other 32x32 instructions.
//
// LDS: per stage 128 rows x 128 bytes of A and of B (128 k of fp8 or 256 k of fp4: the
// geometry is shared, only the k bookkeeping differs), two stages, 64 KB.  Rows are *not*
// padded: a lane reads two 16-byte chunks 32 bytes apart (fp8, two ds_read_b128) or one (fp4)
// per instruction, and the 16-byte chunk c of row r is stored at chunk c ^ key(r),
//   key(r) = (r & 7) ^ ((r >> 3) & 1),
// an xor swizzle.  With 64 banks of 4 bytes the bank group of a 16-byte access is
// 8 * (r & 1) + (c ^ key(r)) of 16.  A ds_read_b128 serves 16 lanes together, rows r .. r+15
// at one c (both formats: the half-wave offset and the MFMA index only change c): rows 0..7
// have distinct keys whose low bit equals r & 1, rows 8..15 distinct keys whose low bit
// differs from r & 1, so the sixteen (r & 1, key) pairs are distinct and the reads are
// conflict-free.  Counted with 32 banks and 8 lanes together the group is c ^ key(r) of 8 and
// rows r .. r+7 have 8 distinct keys: conflict-free as well.  The stage writes (8 lanes cover
// the 8 chunks of a row, the next 8 lanes row r+1) fill one 128-byte half of the banks per
// row and the other half for the next row: conflict-free too, where the padded bf16 layout
// overlaps at the seam.  Against padding the swizzle costs one xor per read address and saves
// 8 KB; the xor folds the half-wave offset into the per-lane term, so it is one VALU
// operation per instruction and operand, next to a 16- or 8-pass MFMA.
//
// Scales do not go through LDS.  A K step is 4 (fp8) or 8 (fp4) blocks per row, one or two
// 32-bit words of SA[M][K/32]; each lane loads the words of its own 2 + 2 rows with the next
// stage's global loads.  The two half-waves supply blocks 2*kk and 2*kk + 1 of instruction kk
// and OPSEL is an immediate, so the word is shifted right by 8 * half once when it is loaded
// and OPSEL is 0 for even kk, 2 for odd kk.
//
// Rows past M, columns past N and bytes past the row are zero-filled in LDS, never read from
// memory.  K is a multiple of 64 and a row starts 16-byte aligned, so a 16-byte chunk is
// wholly inside or wholly outside.
template <int FMT>
__global__ __launch_bounds__(256) void gemm_abft_mx_kernel(const unsigned char* __restrict__ A,
                                                           const unsigned char* __restrict__ B,
                                                           const unsigned char* __restrict__ SA,
                                                           const unsigned char* __restrict__ SB, int M, int N, int K,
                                                           float* __restrict__ colsum, float* __restrict__ rowsum,
                                                           float* __restrict__ C, int poison_i, int poison_j) {
  constexpr bool FP4 = FMT == MXFP4;
  constexpr int CPI = FP4 ? 1 : 2;  // 16-byte chunks per lane and instruction
  constexpr int SW = FP4 ? 2 : 1;   // scale words per row and stage; 2 * SW instructions along k
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * MX_STAGE_BYTES];  // [stage][A, B]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l32 = lane & 31, half = lane >> 5;
  const int row0 = blockIdx.y * TILE, col0 = blockIdx.x * TILE;
  const int KB = FP4 ? K / 2 : K, KS = K / 32;  // bytes and scales per row

  // global -> LDS copy as in the bf16 kernel: 4 chunks per thread per operand, rows lr + 32 q
  // (all with the key of lr), 8 consecutive lanes per 128-byte row segment
  const int lr = t >> 3, kc = t & 7;
  const int wch = kc ^ (lr & 7) ^ ((lr >> 3) & 1);
  u32x4 ga[4], gb[4];
  uint32_t sa[2][SW], sb[2][SW], nsa[2][SW], nsb[2][SW];
  const u32x4 zero = {0u, 0u, 0u, 0u};

#define LOAD_GLOBAL(step)                                                                      \
  do {                                                                                         \
    const int k_ = (step) * MX_ROW_BYTES + kc * 16;                                            \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
      const int ra_ = row0 + lr + 32 * q, rb_ = col0 + lr + 32 * q;                            \
      ga[q] = (ra_ < M && k_ < KB) ? *reinterpret_cast<const u32x4*>(A + static_cast<size_t>(ra_) * KB + k_) : zero; \
      gb[q] = (rb_ < N && k_ < KB) ? *reinterpret_cast<const u32x4*>(B + static_cast<size_t>(rb_) * KB + k_) : zero; \
    }                                                                                          \
    _Pragma("unroll") for (int bl = 0; bl < 2; ++bl)                                           \
      _Pragma("unroll") for (int p = 0; p < SW; ++p) {                                         \
        const int kb_ = ((step) * SW + p) * 4;                                                 \
        nsa[bl][p] = load_scale_word(SA, row0 + wm * 64 + bl * 32 + l32, M, KS, kb_) >> (8 * half); \
        nsb[bl][p] = load_scale_word(SB, col0 + wn * 64 + bl * 32 + l32, N, KS, kb_) >> (8 * half); \
      }                                                                                        \
  } while (0)
#define STORE_LDS(stage)                                                                       \
  do {                                                                                         \
    unsigned char* d_ = lds + (stage) * 2 * MX_STAGE_BYTES + lr * MX_ROW_BYTES + wch * 16;     \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
      *reinterpret_cast<u32x4*>(d_ + 32 * q * MX_ROW_BYTES) = ga[q];                           \
      *reinterpret_cast<u32x4*>(d_ + MX_STAGE_BYTES + 32 * q * MX_ROW_BYTES) = gb[q];          \
    }                                                                                          \
    _Pragma("unroll") for (int bl = 0; bl < 2; ++bl)                                           \
      _Pragma("unroll") for (int p = 0; p < SW; ++p) {                                         \
        sa[bl][p] = nsa[bl][p];                                                                \
        sb[bl][p] = nsb[bl][p];                                                                \
      }                                                                                        \
  } while (0)

  f32x16 acc[2][2];
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int bn = 0; bn < 2; ++bn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bm][bn][r] = 0.0f;

  // the lane's chunk of instruction kk is 2 * CPI * kk + half (+ 2 for fp8's second read),
  // xored with the key of its row: fold half and key into one per-lane term
  const int xs = (l32 & 7) ^ ((l32 >> 3) & 1) ^ half;
  const int nsteps = (KB + MX_ROW_BYTES - 1) / MX_ROW_BYTES;
  LOAD_GLOBAL(0);
  STORE_LDS(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int stage = s & 1;
    const bool more = s + 1 < nsteps;
    const unsigned char* pa = lds + stage * 2 * MX_STAGE_BYTES + (wm * 64 + l32) * MX_ROW_BYTES;
    const unsigned char* pb = lds + stage * 2 * MX_STAGE_BYTES + MX_STAGE_BYTES + (wn * 64 + l32) * MX_ROW_BYTES;
    if (more) LOAD_GLOBAL(s + 1);  // elements and scales in flight while this step multiplies
#pragma unroll
    for (int p = 0; p < SW; ++p) {
      mx_mfma_2x2<FMT, 0>(pa, pb, (4 * p * CPI) ^ xs, sa[0][p], sa[1][p], sb[0][p], sb[1][p], acc);
      mx_mfma_2x2<FMT, 2>(pa, pb, ((4 * p + 2) * CPI) ^ xs, sa[0][p], sa[1][p], sb[0][p], sb[1][p], acc);
    }
    // the other stage was last read in step s-1, before the barrier that ended it; the scale
    // registers of this step are dead from here
    if (more) STORE_LDS(stage ^ 1);
    __syncthreads();
  }
#undef LOAD_GLOBAL
#undef STORE_LDS

  abft_epilogue(acc, reinterpret_cast<float*>(lds), M, N, colsum, rowsum, C, poison_i, poison_j);
}

// ------------------------------------------------------------------------------------------
// The FP64 GEMM on the double-precision matrix path, with a checksum epilogue in double
// ------------------------------------------------------------------------------------------

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int F64_KSTEP = 16;                   // K advance per LDS stage
constexpr int F64_ROW_BYTES = F64_KSTEP * 8;    // 128 B, no padding
constexpr int F64_STAGE_BYTES = TILE * F64_ROW_BYTES;

// The checksum epilogue of the FP64 kernel, from registers: a wave holds its 64x64 quadrant as
// 4x4 blocks of 16x16 accumulators, double r of lane l holding D[4 * r + l / 16][l % 16].
// `red` is 512 doubles of LDS that no wave reads any more.  Element (bm, bn, r) of this lane is
//   row  row0 + wm*64 + bm*16 + 4*r + l/16,   column  col0 + wn*64 + bn*16 + l%16.
// Every sum formed here is an integer below 2^52 (see the header), so the order does not matter.
__device__ __forceinline__ void abft_epilogue_f64(f64x4 (&acc)[4][4], double* red, int M, int N,
                                                  double* __restrict__ colsum, double* __restrict__ rowsum,
                                                  double* __restrict__ C, int poison_i, int poison_j) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l16 = lane & 15, grp = lane >> 4;
  const int tn = blockIdx.x, tm = blockIdx.y;
  const int row0 = tm * TILE, col0 = tn * TILE;
  const int lane_row = row0 + wm * 64 + grp, lane_col = col0 + wn * 64 + l16;
  if (poison_i >= 0) {  // detector self-test: one element off by one
#pragma unroll
    for (int bm = 0; bm < 4; ++bm)
#pragma unroll
      for (int bn = 0; bn < 4; ++bn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool hit = lane_row + bm * 16 + 4 * r == poison_i && lane_col + bn * 16 == poison_j;
          acc[bm][bn][r] += hit ? 1.0 : 0.0;
        }
  }

  // red [0,256): column partials by wm; [256,512): row partials by wn
  // column sums: over this lane's 16 doubles of a block column, then across the four lane groups
#pragma unroll
  for (int bn = 0; bn < 4; ++bn) {
    double cs = 0.0;
#pragma unroll
    for (int bm = 0; bm < 4; ++bm)
#pragma unroll
      for (int r = 0; r < 4; ++r) cs += acc[bm][bn][r];
    cs += __shfl_xor(cs, 16);
    cs += __shfl_xor(cs, 32);
    if (grp == 0) red[wm * TILE + wn * 64 + bn * 16 + l16] = cs;
  }
  // row sums: per double over the four block columns, then a butterfly over the 16 lanes of a group
#pragma unroll
  for (int bm = 0; bm < 4; ++bm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double rs = (acc[bm][0][r] + acc[bm][1][r]) + (acc[bm][2][r] + acc[bm][3][r]);
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) rs += __shfl_xor(rs, off);
      if (l16 == 0) red[2 * TILE + wn * TILE + wm * 64 + bm * 16 + 4 * r + grp] = rs;
    }
  __syncthreads();
  if (t < TILE) {
    if (col0 + t < N) colsum[static_cast<size_t>(tm) * N + col0 + t] = red[t] + red[TILE + t];
  } else {
    const int u = t - TILE;
    if (row0 + u < M) rowsum[static_cast<size_t>(tn) * M + row0 + u] = red[2 * TILE + u] + red[3 * TILE + u];
  }

  if (C != nullptr) {  // --c-out only; the production run never stores M x N
#pragma unroll
    for (int bm = 0; bm < 4; ++bm)
#pragma unroll
      for (int bn = 0; bn < 4; ++bn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = lane_row + bm * 16 + 4 * r, col = lane_col + bn * 16;
          if (row < M && col < N) C[static_cast<size_t>(row) * N + col] = acc[bm][bn][r];
        }
  }
}

// Compiled for gfx950 (-O3, kernel-resource-usage): 222 VGPRs + 0 AGPRs (the 128 accumulator
// registers are VGPRs), 65536 B LDS, 0 scratch, 0 SGPR/VGPR spills; occupancy 2 waves per SIMD,
// asked for by the launch bounds (left alone the compiler takes 216 + 128 at occupancy 1): two
// workgroups per CU, bounded by LDS (2 x 64 KB of 160 KB) and by registers (224 of 256) alike.
//
// The work split is that of the other two: one workgroup (4 waves) per 128x128 tile of C, wave
// w the 64x64 quadrant (w / 2, w % 2), so the 128-row checksum stripes are the same.  A
// quadrant is 4x4 blocks of v_mfma_f64_16x16x4_f64: 16 accumulators of 4 doubles, 128
// registers per lane.
//
// Operand layout of the instruction (CDNA4 ISA guide, matrix arithmetic; settled on the device
// by the one-instruction shape of the tests, with random data): lane l supplies one double,
// A[l % 16][k = l / 16] and B[k = l / 16][l % 16]; accumulator double r of lane l holds
// D[4 * r + l / 16][l % 16].  (Not D[4 * (l / 16) + r][l % 16], the layout of the fp32 16x16
// instructions: a lane group's four doubles are four rows apart, not adjacent.  Products and
// column sums are the same either way; only rows move, so data equal along a column hides it.)
//
// Two k per read.  A sum over k may take the k in any order, here exactly.  A lane reads the
// 16 bytes of k = 2 * (l / 16) and 2 * (l / 16) + 1 of an 8-deep group with one ds_read_b128;
// one instruction then takes every lane's lower double (k = 0, 2, 4, 6 of the group, the same
// for A and B) and the next every upper one (k = 1, 3, 5, 7).  Per 8 k a wave issues 4 + 4
// reads for 32 instructions, and every operand register pair is used four times: the a of a
// block row against the four b, in the order (bm, bn) row by row, so that an accumulator is
// written again only after the 15 other instructions of the sweep.
//
// LDS: per stage 128 rows x 16 k (128 bytes) of A and of B, two stages, 64 KB; the next
// stage's global loads are in flight during the 64 instructions of this one.  Rows are not
// padded; the 16-byte chunk c (two k) of row r is stored at chunk c ^ key(r),
//   key(r) = (r >> 1) & 7,
// an xor swizzle, but not the key of the microscaling kernel.  With 64 banks of 4 bytes a
// 16-byte access at row r, stored chunk p, starts in the 4-bank group 8 * (r & 1) + p of 16.
// A ds_read_b128 is served 16 lanes at a time, and these are not 16 consecutive lanes but
// {0-3, 12-15, 20-23, 24-27}, {4-7, 8-11, 16-19, 28-31} and the same plus 32 (published for
// CDNA3; the counter below says the same of this device).  Such a set is half of the lane
// group l / 16 = g and half of g + 1, g even, and between them each l % 16 once: it reads
// rows r .. r+15 (r a multiple of 16), rows 0-3 and 12-15 at chunk c = 4 * kk + g and rows
// 4-11 at c ^ 1, or the other way round.  So row r reads stored chunk c ^ key(r) ^ m(r),
// m = 0 or 1 and equal for the four rows of an r >> 2.  Among the 8 rows of one parity
// key(r) is each of 0..7 once; m flips its low bit for both rows (4i, 4i + 2, or the odd
// ones) that hold keys 2i and 2i + 1 or for neither, so these 8 rows still read 8 distinct
// chunks, and the two parities start 8 groups apart: sixteen distinct 4-bank groups, every
// bank once, conflict-free.  Sixteen consecutive lanes are the case m = 0.  (The key of the
// microscaling kernel, (r & 7) ^ ((r >> 3) & 1), fails here: rows 0 and 8 then meet at m = 0
// and 1.  Measured with it: 64 conflict cycles per wave and stage.)  The stage writes cost
// nothing extra: 8 consecutive lanes cover the 8 chunks of a row, one 128-byte half of the
// banks, and the next 8 lanes the row after it, the other half; served in the sets above it
// is a half row of each of rows r .. r+3 (chunks 0-3, 4-7, 4-7, 0-3 before the xor), and the
// keys of rows r and r + 2 differ in bit 0 only, which leaves a half row in its half.
// SQ_LDS_BANK_CONFLICT over the whole kernel (2048 x 2048 x 1024, counters only): 0 cycles.
// The swizzle is one xor per stage in the read address (key and l / 16 fold into one per-lane
// term), next to 64 matrix instructions.
//
// Rows past M, columns past N and k past K are zero-filled in LDS, never read from memory.
// K is a multiple of 4 and a row starts 32-byte aligned, so a 16-byte chunk of two doubles is
// wholly inside a row or wholly outside it.
__global__ __launch_bounds__(256, 2) void gemm_abft_f64_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                            int M, int N, int K, double* __restrict__ colsum,
                                                            double* __restrict__ rowsum, double* __restrict__ C,
                                                            int poison_i, int poison_j) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * F64_STAGE_BYTES];  // [stage][A, B]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l16 = lane & 15, grp = lane >> 4;
  const int row0 = blockIdx.y * TILE, col0 = blockIdx.x * TILE;

  // global -> LDS copy as in the other kernels: a stage tile is 1024 16-byte chunks, 4 per
  // thread per operand, rows lr + 32 q (all with the key of lr), 8 consecutive lanes per row
  const int lr = t >> 3, kc = t & 7;
  const int wch = kc ^ ((lr >> 1) & 7);
  u32x4 ga[4], gb[4];
  const u32x4 zero = {0u, 0u, 0u, 0u};

#define LOAD_GLOBAL(k0)                                                                        \
  do {                                                                                         \
    const int k_ = (k0) + kc * 2;                                                              \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
      const int ra_ = row0 + lr + 32 * q, rb_ = col0 + lr + 32 * q;                            \
      ga[q] = (ra_ < M && k_ < K) ? *reinterpret_cast<const u32x4*>(A + static_cast<size_t>(ra_) * K + k_) : zero; \
      gb[q] = (rb_ < N && k_ < K) ? *reinterpret_cast<const u32x4*>(B + static_cast<size_t>(rb_) * K + k_) : zero; \
    }                                                                                          \
  } while (0)
#define STORE_LDS(stage)                                                                       \
  do {                                                                                         \
    unsigned char* d_ = lds + (stage) * 2 * F64_STAGE_BYTES + lr * F64_ROW_BYTES + wch * 16;   \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
      *reinterpret_cast<u32x4*>(d_ + 32 * q * F64_ROW_BYTES) = ga[q];                          \
      *reinterpret_cast<u32x4*>(d_ + F64_STAGE_BYTES + 32 * q * F64_ROW_BYTES) = gb[q];        \
    }                                                                                          \
  } while (0)

  f64x4 acc[4][4];
#pragma unroll
  for (int bm = 0; bm < 4; ++bm)
#pragma unroll
    for (int bn = 0; bn < 4; ++bn)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[bm][bn][r] = 0.0;

  // the lane's chunk of group kk is 4 * kk + grp, xored with the key of its row (that of l16,
  // the block rows being multiples of 16): 4 * kk and grp share no bit, so it is (4 * kk) ^ xs
  const int xs = (l16 >> 1) ^ grp;
  const int nsteps = (K + F64_KSTEP - 1) / F64_KSTEP;
  LOAD_GLOBAL(0);
  STORE_LDS(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int stage = s & 1;
    const bool more = s + 1 < nsteps;
    if (more) LOAD_GLOBAL((s + 1) * F64_KSTEP);  // in flight while this step multiplies
    const unsigned char* pa = lds + stage * 2 * F64_STAGE_BYTES + (wm * 64 + l16) * F64_ROW_BYTES;
    const unsigned char* pb = lds + stage * 2 * F64_STAGE_BYTES + F64_STAGE_BYTES + (wn * 64 + l16) * F64_ROW_BYTES;
#pragma unroll
    for (int kk = 0; kk < F64_KSTEP / 8; ++kk) {
      const int off = ((4 * kk) ^ xs) * 16;
      f64x2 a[4], b[4];
#pragma unroll
      for (int bl = 0; bl < 4; ++bl) {
        a[bl] = *reinterpret_cast<const f64x2*>(pa + bl * 16 * F64_ROW_BYTES + off);
        b[bl] = *reinterpret_cast<const f64x2*>(pb + bl * 16 * F64_ROW_BYTES + off);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)  // the even k of the group, then the odd
#pragma unroll
        for (int bm = 0; bm < 4; ++bm)
#pragma unroll
          for (int bn = 0; bn < 4; ++bn)
            acc[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bm][h], b[bn][h], acc[bm][bn], 0, 0, 0);
    }
    // the other stage was last read in step s-1, before the barrier that ended it
    if (more) STORE_LDS(stage ^ 1);
    __syncthreads();
  }
#undef LOAD_GLOBAL
#undef STORE_LDS

  abft_epilogue_f64(acc, reinterpret_cast<double*>(lds), M, N, colsum, rowsum, C, poison_i, poison_j);
}

// ------------------------------------------------------------------------------------------
// The INT8 GEMM on the integer matrix path, with a checksum epilogue in int64
// ------------------------------------------------------------------------------------------

typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int I8_TILE_M = 128, I8_TILE_N = 256;  // C tile per workgroup: 2 x 2 waves of 64 x 128
constexpr int I8_KSTEP = 64;                     // K advance per LDS stage: a stage row is 64 bytes, no padding
constexpr int I8_CPR = I8_KSTEP / 16;            // 16-byte chunks per stage row, and lanes that copy one
constexpr int I8_RPS = 256 / I8_CPR;             // rows the 256 threads copy at once
constexpr int I8_A_BYTES = I8_TILE_M * I8_KSTEP;
constexpr int I8_STAGE_BYTES = (I8_TILE_M + I8_TILE_N) * I8_KSTEP;

// the xor swizzle of a stage row: chunk c of row r is stored at chunk c ^ i8_key(r)
__device__ __forceinline__ int i8_key(int r) { return (r >> 2) & (I8_CPR - 1); }

// The checksum epilogue of the INT8 kernel, from registers: a wave holds its 64x128 block as 2x4
// blocks of 32x32 accumulators, register r of lane l holding D[8 * (r / 4) + 4 * (l / 32) + r % 4][l % 32].
// Element (bm, bn, r) of this lane is
//   row  row0 + wm*64 + bm*32 + 8*(r/4) + 4*half + r%4,   column  col0 + wn*128 + bn*32 + l32.
// An element is at most 2^30 in magnitude and a checksum of 128 of them 2^37, so every sum here
// is int64.  The stripes stay 128 wide: the column checksums of the workgroup's 128 rows go to
// stripe tm (two wm partials per column), and a wave's row sums over its four column blocks are
// already the whole checksum of stripe 2 * tn + wn, which exists only where it starts inside N.
// `red` is 768 int64 of LDS that no wave reads any more.
__device__ __forceinline__ void abft_epilogue_i8(i32x16 (&acc)[2][4], long long* red, int M, int N,
                                                 long long* __restrict__ colsum, long long* __restrict__ rowsum,
                                                 int* __restrict__ C, int poison_i, int poison_j) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l32 = lane & 31, half = lane >> 5;
  const int tn = blockIdx.x, tm = blockIdx.y;
  const int row0 = tm * I8_TILE_M, col0 = tn * I8_TILE_N;
  const int lane_row = row0 + wm * 64 + 4 * half, lane_col = col0 + wn * 128 + l32;
  if (poison_i >= 0) {  // detector self-test: one element off by one
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int bn = 0; bn < 4; ++bn)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool hit = lane_row + bm * 32 + 8 * (r >> 2) + (r & 3) == poison_i && lane_col + bn * 32 == poison_j;
          acc[bm][bn][r] += hit ? 1 : 0;
        }
  }

  // red [0,512): column partials by wm, 256 columns each; [512,768): row sums by wn, 128 rows each
  // One sweep over the registers widens each to int64 once, for both sums (widened twice, in a
  // sweep per sum, the compiler keeps all 128 widened values and spills).
  // row sums: per register over the four column blocks, then a butterfly over the 32 lanes of a
  // half-wave (a 64-bit shuffle is two 32-bit ones), after which every lane holds the sum; lane
  // l32 keeps that of (bm, r) = (l32 / 16, l32 % 16), so a half-wave's 32 rows are one store per
  // lane and no branch splits the sweep.
  // column sums: over this lane's 32 registers of a block column, then across the two half-waves;
  // both halves then hold all four, and half h stores those of blocks 2h and 2h + 1.
  long long cs[4] = {0, 0, 0, 0}, mine = 0;
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      long long rs = 0;
#pragma unroll
      for (int bn = 0; bn < 4; ++bn) {
        const long long v = acc[bm][bn][r];
        cs[bn] += v;
        rs += v;
      }
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) rs += __shfl_xor(rs, off);
      mine = l32 == bm * 16 + r ? rs : mine;
    }
  red[2 * I8_TILE_N + wn * I8_TILE_M + wm * 64 + (l32 >> 4) * 32 + 8 * ((l32 >> 2) & 3) + 4 * half + (l32 & 3)] = mine;
#pragma unroll
  for (int bn = 0; bn < 4; ++bn) cs[bn] += __shfl_xor(cs[bn], 32);
  const long long lo0 = cs[0], lo1 = cs[1], hi0 = cs[2], hi1 = cs[3];  // chosen as values: no indexed array in scratch
  long long* const cred = red + wm * I8_TILE_N + wn * 128 + 2 * half * 32 + l32;
  cred[0] = half ? hi0 : lo0;
  cred[32] = half ? hi1 : lo1;
  __syncthreads();
  if (col0 + t < N) colsum[static_cast<size_t>(tm) * N + col0 + t] = red[t] + red[I8_TILE_N + t];
  const int stripe = 2 * tn + (t >> 7), u = t & 127;  // thread t also owns row u of the stripe of wn = t / 128
  if (stripe * TILE < N && row0 + u < M) rowsum[static_cast<size_t>(stripe) * M + row0 + u] = red[2 * I8_TILE_N + t];

  if (C != nullptr) {  // --c-out only; the production run never stores M x N
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int bn = 0; bn < 4; ++bn)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = lane_row + bm * 32 + 8 * (r >> 2) + (r & 3), col = lane_col + bn * 32;
          if (row < M && col < N) C[static_cast<size_t>(row) * N + col] = acc[bm][bn][r];
        }
  }
}

// Compiled for gfx950 (-O3, kernel-resource-usage): 204 VGPRs + 0 AGPRs (the 128 accumulator
// registers are VGPRs), 49152 B LDS, 0 scratch, 0 SGPR/VGPR spills; occupancy 2 waves per SIMD,
// asked for by the launch bounds: two workgroups per CU, bounded by registers (204 of 256; the
// LDS, 2 x 48 KB of 160 KB, would admit three).
//
// The work split is not that of the other three.  One workgroup (4 waves, 2 x 2) owns a 128x256
// tile of C and wave w the 64x128 block (w / 2, w % 2) as 2x4 blocks of v_mfma_i32_32x32x32_i8:
// 8 accumulators of 16 registers, 128 per lane.  Per 32 k a wave reads 2 operands of A and 4 of
// B (one ds_read_b128 each, 16 int8 per lane) for 8 matrix instructions, 0.75 LDS reads per
// instruction where the 2x2 layout has 1, and every operand register is used 4 or 2 times.  A
// 128x256 tile also takes (128 + 256) / (2 * 128 * 256) bytes of global and L2 traffic per
// product, a third less than 128x128.  The grid is ceil(N / 256) x ceil(M / 128); the checksum
// stripes stay 128 wide (see the epilogue), so the expectation, verdict and locate kernels and
// the 128x128 tile index of a mismatch record are shared with the other formats.  An
// accumulator is written again only after the 7 other instructions of the sweep.
//
// Operand layout of the instruction (CDNA4 ISA guide, matrix arithmetic, by analogy with the
// bf16 instruction; the device agreed: the one-instruction shape of the tests, 32x32x32 on
// random bytes, is exact against int64, and so are the larger ones): lane l supplies row (A) or column (B) l % 32 and the 16
// consecutive k values 16 * (l / 32) .. + 15, k ascending from the low byte of register 0;
// accumulator register r of lane l holds D[8 * (r / 4) + 4 * (l / 32) + r % 4][l % 32].
//
// LDS: per stage 128 rows of A and 256 of B, 64 k = 64 bytes each, 24 KB; two stages, 48 KB.
// The next stage's global loads (6 x 16 bytes per thread: 4 consecutive lanes cover a row, the
// 256 threads 64 rows, 2 sweeps of A and 4 of B) are in flight during the 16 matrix
// instructions of this one.  The deeper stage, 128-byte rows (key (r >> 1) & 7, 12 staging
// registers), halves the barriers but takes 96 KB, one workgroup per CU; the compiler then gives
// 194 VGPRs + 128 AGPRs at occupancy 1.  Measured alternating at 8192^3, three rounds: 1767.4,
// 1766.5, 1767.1 TOP/s with 64-byte rows against 1486.9, 1488.8, 1492.3 with 128-byte rows.  A
// second workgroup to run while one waits at its barrier is worth more than half the barriers,
// so the 64-byte stage is the one kept.
//
// Rows are not padded; the 16-byte chunk c of row r is stored at chunk c ^ key(r),
//   key(r) = (r >> 2) & 3.
// With 64 banks of 4 bytes four 64-byte rows fill the banks once, and a 16-byte access at row r,
// stored chunk p, starts in the 4-bank group 4 * (r & 3) + p of 16.  A ds_read_b128 is served 16
// lanes at a time, in the sets {0-3, 12-15, 20-23, 24-27}, {4-7, 8-11, 16-19, 28-31} and the
// same plus 32 (see the FP64 kernel).  A set lies in one half-wave, so all its lanes read one k
// chunk c, of four groups of four rows; the four rows of a group have the four r & 3 and one
// key, and the keys of the groups are (r >> 2) & 3 = {0, 3, 1, 2} for the first set and
// {1, 2, 0, 3} for the second: sixteen distinct 4-bank groups, conflict-free.  The stage
// writes are 4 lanes per row, so a set covers all four chunks of four rows, rows {0, 3, 5, 6}
// or {1, 2, 4, 7} of eight, with four distinct r & 3: conflict-free too.
// SQ_LDS_BANK_CONFLICT over the whole kernel (2048 x 2048 x 1024, counters only): 2048 cycles,
// 4 per wave over 16 stages of 18 LDS accesses each.  A conflict in the loop would cost at
// least one cycle per stage, 16 per wave, so the loop has none; the 4 are outside it, where
// the epilogue stores its 8-byte sums.
//
// Rows past M, columns past N and k past K are zero-filled in LDS, never read from memory.
// K is a multiple of 32 and a row starts 16-byte aligned, so a 16-byte chunk is wholly inside a
// row or wholly outside it.
__global__ __launch_bounds__(256, 2) void gemm_abft_i8_kernel(const unsigned char* __restrict__ A,
                                                              const unsigned char* __restrict__ B, int M, int N, int K,
                                                              long long* __restrict__ colsum, long long* __restrict__ rowsum,
                                                              int* __restrict__ C, int poison_i, int poison_j) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * I8_STAGE_BYTES];  // [stage][A, B]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int l32 = lane & 31, half = lane >> 5;
  const int row0 = blockIdx.y * I8_TILE_M, col0 = blockIdx.x * I8_TILE_N;

  // global -> LDS copy: rows lr + 64 q, all with the key of lr
  constexpr int QA = I8_TILE_M / I8_RPS, QB = I8_TILE_N / I8_RPS;
  const int lr = t / I8_CPR, kc = t % I8_CPR;
  const int wch = kc ^ i8_key(lr);
  u32x4 ga[QA], gb[QB];
  const u32x4 zero = {0u, 0u, 0u, 0u};

#define LOAD_GLOBAL(k0)                                                                        \
  do {                                                                                         \
    const int k_ = (k0) + kc * 16;                                                             \
    _Pragma("unroll") for (int q = 0; q < QA; ++q) {                                           \
      const int ra_ = row0 + lr + I8_RPS * q;                                                  \
      ga[q] = (ra_ < M && k_ < K) ? *reinterpret_cast<const u32x4*>(A + static_cast<size_t>(ra_) * K + k_) : zero; \
    }                                                                                          \
    _Pragma("unroll") for (int q = 0; q < QB; ++q) {                                           \
      const int rb_ = col0 + lr + I8_RPS * q;                                                  \
      gb[q] = (rb_ < N && k_ < K) ? *reinterpret_cast<const u32x4*>(B + static_cast<size_t>(rb_) * K + k_) : zero; \
    }                                                                                          \
  } while (0)
#define STORE_LDS(stage)                                                                       \
  do {                                                                                         \
    unsigned char* d_ = lds + (stage) * I8_STAGE_BYTES + lr * I8_KSTEP + wch * 16;             \
    _Pragma("unroll") for (int q = 0; q < QA; ++q)                                             \
      *reinterpret_cast<u32x4*>(d_ + I8_RPS * q * I8_KSTEP) = ga[q];                           \
    _Pragma("unroll") for (int q = 0; q < QB; ++q)                                             \
      *reinterpret_cast<u32x4*>(d_ + I8_A_BYTES + I8_RPS * q * I8_KSTEP) = gb[q];              \
  } while (0)

  i32x16 acc[2][4];
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int bn = 0; bn < 4; ++bn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bm][bn][r] = 0;

  // the lane's chunk of instruction kk is 2 * kk + half, xored with the key of its row (that of
  // l32, the block rows being multiples of 32): 2 * kk and half share no bit, so it is (2 * kk) ^ xs
  const int xs = i8_key(l32) ^ half;
  const int nsteps = (K + I8_KSTEP - 1) / I8_KSTEP;
  LOAD_GLOBAL(0);
  STORE_LDS(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int stage = s & 1;
    const bool more = s + 1 < nsteps;
    if (more) LOAD_GLOBAL((s + 1) * I8_KSTEP);  // in flight while this step multiplies
    const unsigned char* pa = lds + stage * I8_STAGE_BYTES + (wm * 64 + l32) * I8_KSTEP;
    const unsigned char* pb = lds + stage * I8_STAGE_BYTES + I8_A_BYTES + (wn * 128 + l32) * I8_KSTEP;
#pragma unroll
    for (int kk = 0; kk < I8_KSTEP / 32; ++kk) {
      const int off = ((2 * kk) ^ xs) * 16;
      i32x4 a[2], b[4];
#pragma unroll
      for (int bl = 0; bl < 2; ++bl) a[bl] = *reinterpret_cast<const i32x4*>(pa + bl * 32 * I8_KSTEP + off);
#pragma unroll
      for (int bl = 0; bl < 4; ++bl) b[bl] = *reinterpret_cast<const i32x4*>(pb + bl * 32 * I8_KSTEP + off);
#pragma unroll
      for (int bm = 0; bm < 2; ++bm)
#pragma unroll
        for (int bn = 0; bn < 4; ++bn)
          acc[bm][bn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[bm], b[bn], acc[bm][bn], 0, 0, 0);
    }
    // the other stage was last read in step s-1, before the barrier that ended it
    if (more) STORE_LDS(stage ^ 1);
    __syncthreads();
  }
#undef LOAD_GLOBAL
#undef STORE_LDS

  abft_epilogue_i8(acc, reinterpret_cast<long long*>(lds), M, N, colsum, rowsum, C, poison_i, poison_j);
}

// ------------------------------------------------------------------------------------------
// Expected checksums, in integer arithmetic
// ------------------------------------------------------------------------------------------

__device__ static inline int bf16_int(uint32_t bits16) {  // exact for the small integers used here
  return static_cast<int>(__uint_as_float(bits16 << 16));
}

// e[s][k] = sum over the rows of stripe s (128 rows, fewer in the last) of X[row][k]
__global__ __launch_bounds__(256) void stripe_sum_kernel(const uint16_t* __restrict__ X, int rows, int K,
                                                         int* __restrict__ e) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (k >= K) return;
  const int end = min(rows, (s + 1) * TILE);
  int sum = 0;
  for (int i = s * TILE; i < end; ++i) sum += bf16_int(X[static_cast<size_t>(i) * K + k]);
  e[static_cast<size_t>(s) * K + k] = sum;
}

// out[s][y] = sum_k e[s][k] * Y[y][k]: one wave per (y, s), 8 k per lane per trip
__global__ __launch_bounds__(256) void expect_kernel(const int* __restrict__ e, int stripes, const uint16_t* __restrict__ Y,
                                                     int rows_y, int K, int* __restrict__ out) {
  const int lane = threadIdx.x & 63, s = blockIdx.y * 4 + (threadIdx.x >> 6), y = blockIdx.x;
  if (s >= stripes) return;  // whole waves leave; no barrier below
  const uint16_t* yr = Y + static_cast<size_t>(y) * K;
  const int* er = e + static_cast<size_t>(s) * K;
  int sum = 0;
  for (int k = lane * 8; k < K; k += 512) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(yr + k);
    const i32x4 e0 = *reinterpret_cast<const i32x4*>(er + k), e1 = *reinterpret_cast<const i32x4*>(er + k + 4);
    sum += e0[0] * bf16_int(v[0] & 0xffffu) + e0[1] * bf16_int(v[0] >> 16) + e0[2] * bf16_int(v[1] & 0xffffu) +
           e0[3] * bf16_int(v[1] >> 16) + e1[0] * bf16_int(v[2] & 0xffffu) + e1[1] * bf16_int(v[2] >> 16) +
           e1[2] * bf16_int(v[3] & 0xffffu) + e1[3] * bf16_int(v[3] >> 16);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) out[static_cast<size_t>(s) * rows_y + y] = sum;
}

// The microscaling siblings decode element and scale with integer operations into units of 1
// (E4M3) or 1/2 (E2M1) per operand; a checksum of products is then in units of 1 or 1/4.
template <int FMT>
__device__ static inline int mx_units(uint32_t code) {
  if (FMT == MXFP8) {  // s eeee mmm, bias 7: (8 + m) * 2^(e - 10), an integer for the bytes used here
    const int e = (code >> 3) & 15, mag = e ? ((8 | (code & 7)) << e) >> 10 : 0;
    return (code & 0x80u) ? -mag : mag;
  }
  // s ee m, bias 1, in halves: m when e == 0 (the subnormal), else (2 + m) * 2^(e - 1)
  const int e = (code >> 1) & 3, m = code & 1, mag = e ? (2 | m) << (e - 1) : m;
  return (code & 8u) ? -mag : mag;
}

template <int FMT>
__global__ __launch_bounds__(256) void stripe_sum_mx_kernel(const unsigned char* __restrict__ X,
                                                            const unsigned char* __restrict__ S, int rows, int K,
                                                            int* __restrict__ e) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (k >= K) return;
  const int end = min(rows, (s + 1) * TILE);
  int sum = 0;
  for (int i = s * TILE; i < end; ++i) {
    const size_t at = static_cast<size_t>(i) * K + k;
    const uint32_t code = FMT == MXFP8 ? X[at] : (X[at / 2] >> (4 * (k & 1))) & 15u;
    sum += mx_units<FMT>(code) * (1 << (S[at / 32] - 127));
  }
  e[static_cast<size_t>(s) * K + k] = sum;
}

// one wave per (y, s) as in expect_kernel; a lane's 8 k lie in one scale block
template <int FMT>
__global__ __launch_bounds__(256) void expect_mx_kernel(const int* __restrict__ e, int stripes,
                                                        const unsigned char* __restrict__ Y,
                                                        const unsigned char* __restrict__ SY, int rows_y, int K,
                                                        int* __restrict__ out) {
  constexpr int BITS = FMT == MXFP8 ? 8 : 4;
  const int lane = threadIdx.x & 63, s = blockIdx.y * 4 + (threadIdx.x >> 6), y = blockIdx.x;
  if (s >= stripes) return;  // whole waves leave; no barrier below
  const unsigned char* yr = Y + static_cast<size_t>(y) * K * BITS / 8;
  const unsigned char* sr = SY + static_cast<size_t>(y) * (K / 32);
  const int* er = e + static_cast<size_t>(s) * K;
  int sum = 0;
  for (int k = lane * 8; k < K; k += 512) {
    uint64_t v = *reinterpret_cast<const uint32_t*>(yr + k * BITS / 8);
    if (FMT == MXFP8) v |= static_cast<uint64_t>(*reinterpret_cast<const uint32_t*>(yr + k + 4)) << 32;
    int part = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) part += er[k + j] * mx_units<FMT>(static_cast<uint32_t>(v >> (BITS * j)) & ((1u << BITS) - 1u));
    sum += part * (1 << (sr[k >> 5] - 127));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) out[static_cast<size_t>(s) * rows_y + y] = sum;
}

// The FP64 siblings share nothing with the double-precision unit: a double is decoded to its
// integer from the bit pattern (sign, exponent, shifted significand) with integer operations,
// never a conversion, so that no fault of that unit can cancel on both sides of the ==.
// False when the double holds no integer of magnitude below 2^53: a fraction, an infinity, a NaN.
__host__ __device__ static inline bool f64_int(uint64_t bits, long long* out) {
  const int e = static_cast<int>(bits >> 52) & 0x7ff;
  const uint64_t frac = bits & ((1ull << 52) - 1);
  *out = 0;
  if (e == 0) return frac == 0;             // +-0; a subnormal is a fraction
  if (e < 1023 || e > 1075) return false;   // below 1; 2^53 and above, infinity, NaN
  const uint64_t sig = (1ull << 52) | frac;  // the value is sig * 2^(e - 1075)
  const int drop = 1075 - e;                 // 0 .. 52
  if (sig & ((1ull << drop) - 1)) return false;
  const long long mag = static_cast<long long>(sig >> drop);
  *out = (bits >> 63) ? -mag : mag;
  return true;
}

__device__ static inline int f64_elem(uint64_t bits) {  // an input element: validated or generated, |x| <= 65535
  long long v;
  f64_int(bits, &v);
  return static_cast<int>(v);
}

// as stripe_sum_kernel; a stripe sum is at most 65535 * 128 < 2^23
__global__ __launch_bounds__(256) void stripe_sum_f64_kernel(const uint64_t* __restrict__ X, int rows, int K,
                                                             int* __restrict__ e) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (k >= K) return;
  const int end = min(rows, (s + 1) * TILE);
  int sum = 0;
  for (int i = s * TILE; i < end; ++i) sum += f64_elem(X[static_cast<size_t>(i) * K + k]);
  e[static_cast<size_t>(s) * K + k] = sum;
}

// one wave per (y, s) as in expect_kernel, 2 k per lane per trip (K is even); the sum is below
// 2^23 * 2^16 * K <= 2^52 and is kept in int64
__global__ __launch_bounds__(256) void expect_f64_kernel(const int* __restrict__ e, int stripes,
                                                         const uint64_t* __restrict__ Y, int rows_y, int K,
                                                         long long* __restrict__ out) {
  const int lane = threadIdx.x & 63, s = blockIdx.y * 4 + (threadIdx.x >> 6), y = blockIdx.x;
  if (s >= stripes) return;  // whole waves leave; no barrier below
  const uint64_t* yr = Y + static_cast<size_t>(y) * K;
  const int* er = e + static_cast<size_t>(s) * K;
  long long sum = 0;
  for (int k = lane * 2; k < K; k += 128) {
    const u64x2 v = *reinterpret_cast<const u64x2*>(yr + k);
    sum += static_cast<long long>(er[k]) * f64_elem(v[0]) + static_cast<long long>(er[k + 1]) * f64_elem(v[1]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) out[static_cast<size_t>(s) * rows_y + y] = sum;
}

// The INT8 siblings: plain integer multiply-adds.  As stripe_sum_kernel, four k per thread (K is
// a multiple of 32); a stripe sum is at most 128 * 128 = 2^14.
__global__ __launch_bounds__(256) void stripe_sum_i8_kernel(const unsigned char* __restrict__ X, int rows, int K,
                                                            int* __restrict__ e) {
  const int k = (blockIdx.x * blockDim.x + threadIdx.x) * 4, s = blockIdx.y;
  if (k >= K) return;
  const int end = min(rows, (s + 1) * TILE);
  i32x4 sum = {0, 0, 0, 0};
  for (int i = s * TILE; i < end; ++i) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(X + static_cast<size_t>(i) * K + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] += static_cast<int8_t>(v >> (8 * j));
  }
  *reinterpret_cast<i32x4*>(e + static_cast<size_t>(s) * K + k) = sum;
}

// one wave per (y, s) as in expect_kernel, 16 k per lane per trip; a trip adds 16 products of
// at most 2^14 * 2^7 in int32, the sum over K is at most 2^37 and is kept in int64
__global__ __launch_bounds__(256) void expect_i8_kernel(const int* __restrict__ e, int stripes,
                                                        const unsigned char* __restrict__ Y, int rows_y, int K,
                                                        long long* __restrict__ out) {
  const int lane = threadIdx.x & 63, s = blockIdx.y * 4 + (threadIdx.x >> 6), y = blockIdx.x;
  if (s >= stripes) return;  // whole waves leave; no barrier below
  const unsigned char* yr = Y + static_cast<size_t>(y) * K;
  const int* er = e + static_cast<size_t>(s) * K;
  long long sum = 0;
  for (int k = lane * 16; k < K; k += 1024) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(yr + k);
    int part = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const i32x4 eq = *reinterpret_cast<const i32x4*>(er + k + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) part += eq[j] * static_cast<int8_t>(v[q] >> (8 * j));
    }
    sum += part;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) out[static_cast<size_t>(s) * rows_y + y] = sum;
}

constexpr int MAX_RECORDS = 16;

struct Suspect {  // one checksum that disagrees
  int stripe, index;
  double delta;
};
struct GemmRecord {
  int kind;  // 0 element, 1 row, 2 column
  int i, j, tile;
  double delta;
};
struct GemmResult {
  unsigned int count, ncol, nrow, nrec;
  Suspect col[MAX_RECORDS], row[MAX_RECORDS];
  GemmRecord rec[MAX_RECORDS];
};

__global__ __launch_bounds__(256) void verify_kernel(const float* __restrict__ colsum, const int* __restrict__ colexp,
                                                     size_t ncol, int N, const float* __restrict__ rowsum,
                                                     const int* __restrict__ rowexp, size_t nrow, int M, float unit,
                                                     GemmResult* res) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t x = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; x < ncol + nrow; x += stride) {
    const bool is_col = x < ncol;
    const size_t y = is_col ? x : x - ncol;
    const float got = (is_col ? colsum[y] : rowsum[y]) * unit;  // in the units of `want`: exact, a power of two
    const float want = static_cast<float>(is_col ? colexp[y] : rowexp[y]);
    if (got == want) continue;  // a NaN is a mismatch
    atomicAdd(&res->count, 1u);
    const unsigned int slot = atomicAdd(is_col ? &res->ncol : &res->nrow, 1u);
    if (slot < MAX_RECORDS) {
      const int width = is_col ? N : M;
      Suspect sus = {static_cast<int>(y / width), static_cast<int>(y % width), (got - want) / unit};
      (is_col ? res->col : res->row)[slot] = sus;
    }
  }
}

// The FP64 sibling: double sums against int64 expectations.  The sum is decoded like the inputs
// and the == is on integers, so a sum that is no integer (a fraction, a NaN) is a mismatch too;
// only the delta of the report is formed in double.
__global__ __launch_bounds__(256) void verify_f64_kernel(const double* __restrict__ colsum,
                                                         const long long* __restrict__ colexp, size_t ncol, int N,
                                                         const double* __restrict__ rowsum,
                                                         const long long* __restrict__ rowexp, size_t nrow, int M,
                                                         GemmResult* res) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t x = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; x < ncol + nrow; x += stride) {
    const bool is_col = x < ncol;
    const size_t y = is_col ? x : x - ncol;
    const double got = is_col ? colsum[y] : rowsum[y];
    const long long want = is_col ? colexp[y] : rowexp[y];
    long long have;
    if (f64_int(static_cast<uint64_t>(__double_as_longlong(got)), &have) && have == want) continue;
    atomicAdd(&res->count, 1u);
    const unsigned int slot = atomicAdd(is_col ? &res->ncol : &res->nrow, 1u);
    if (slot < MAX_RECORDS) {
      const int width = is_col ? N : M;
      Suspect sus = {static_cast<int>(y / width), static_cast<int>(y % width), got - static_cast<double>(want)};
      (is_col ? res->col : res->row)[slot] = sus;
    }
  }
}

// The INT8 sibling: int64 sums against int64 expectations; only the delta of the report is a double.
__global__ __launch_bounds__(256) void verify_i64_kernel(const long long* __restrict__ colsum,
                                                         const long long* __restrict__ colexp, size_t ncol, int N,
                                                         const long long* __restrict__ rowsum,
                                                         const long long* __restrict__ rowexp, size_t nrow, int M,
                                                         GemmResult* res) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t x = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; x < ncol + nrow; x += stride) {
    const bool is_col = x < ncol;
    const size_t y = is_col ? x : x - ncol;
    const long long got = is_col ? colsum[y] : rowsum[y], want = is_col ? colexp[y] : rowexp[y];
    if (got == want) continue;
    atomicAdd(&res->count, 1u);
    const unsigned int slot = atomicAdd(is_col ? &res->ncol : &res->nrow, 1u);
    if (slot < MAX_RECORDS) {
      const int width = is_col ? N : M;
      Suspect sus = {static_cast<int>(y / width), static_cast<int>(y % width), static_cast<double>(got - want)};
      (is_col ? res->col : res->row)[slot] = sus;
    }
  }
}

// A wrong element C[i][j] shows as one column mismatch (stripe i/128, j) and one row mismatch
// (stripe j/128, i): where such a pair intersects, name the element.  One thread; <= 16 x 16.
__global__ void locate_kernel(GemmResult* res, int tiles_n) {
  const int nc = min(res->ncol, static_cast<unsigned int>(MAX_RECORDS));
  const int nr = min(res->nrow, static_cast<unsigned int>(MAX_RECORDS));
  bool row_used[MAX_RECORDS] = {};
  int n = 0;
  for (int c = 0; c < nc && n < MAX_RECORDS; ++c) {
    const int tm = res->col[c].stripe, j = res->col[c].index;
    int hit = -1;
    for (int r = 0; r < nr && hit < 0; ++r)
      if (!row_used[r] && res->row[r].index / TILE == tm && res->row[r].stripe == j / TILE) hit = r;
    GemmRecord rec = {2, tm, j, tm * tiles_n + j / TILE, res->col[c].delta};  // column: i is the stripe
    if (hit >= 0) {
      row_used[hit] = true;
      rec.kind = 0;
      rec.i = res->row[hit].index;
    }
    res->rec[n++] = rec;
  }
  for (int r = 0; r < nr && n < MAX_RECORDS; ++r) {
    if (row_used[r]) continue;
    const int tn = res->row[r].stripe, i = res->row[r].index;
    GemmRecord rec = {1, i, tn, (i / TILE) * tiles_n + tn, res->row[r].delta};  // row: j is the stripe
    res->rec[n++] = rec;
  }
  res->nrec = n;
}

// ------------------------------------------------------------------------------------------
// HBM moving inversions
// ------------------------------------------------------------------------------------------

struct HbmRecord {
  unsigned long long offset;
  uint32_t expected, got;
};
struct HbmResult {
  unsigned long long count;
  unsigned int nrec;
  HbmRecord rec[MAX_RECORDS];
};

// What pass `pass` leaves in 32-bit word `w`: a hash of the address (a stuck or aliased address
// line gives wrong data, not right data in the wrong place), complemented on odd passes.
__host__ __device__ static inline uint32_t hbm_pattern(uint64_t w, uint32_t seed, uint32_t pass) {
  const uint32_t h = mix32(static_cast<uint32_t>(w) ^ mix32(static_cast<uint32_t>(w >> 32) + seed + (pass >> 1) * 0x9e3779b9u));
  return (pass & 1u) ? ~h : h;
}

// One sweep over n16 16-byte words: check against `check_pass` (< 0: none) and store
// `write_pass` (< 0: none).  Non-temporal both ways: the data is touched once per sweep.
__global__ __launch_bounds__(256) void hbm_sweep_kernel(u32x4* __restrict__ p, size_t n16, uint32_t seed, int check_pass,
                                                        int write_pass, HbmResult* res) {
  __shared__ unsigned int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  unsigned int mine = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n16; i += stride) {
    const uint64_t w = static_cast<uint64_t>(i) * 4;
    if (check_pass >= 0) {
      const u32x4 got = __builtin_nontemporal_load(p + i);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t want = hbm_pattern(w + c, seed, static_cast<uint32_t>(check_pass));
        if (got[c] != want) {
          ++mine;
          if (__atomic_load_n(&res->nrec, __ATOMIC_RELAXED) < MAX_RECORDS) {
            const unsigned int slot = atomicAdd(&res->nrec, 1u);
            if (slot < MAX_RECORDS) {
              HbmRecord rec = {(w + c) * 4ull, want, got[c]};
              res->rec[slot] = rec;
            }
          }
        }
      }
    }
    if (write_pass >= 0) {
      u32x4 v;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = hbm_pattern(w + c, seed, static_cast<uint32_t>(write_pass));
      __builtin_nontemporal_store(v, p + i);
    }
  }
  if (mine) atomicAdd(&bad, mine);
  __syncthreads();
  if (threadIdx.x == 0 && bad) atomicAdd(&res->count, static_cast<unsigned long long>(bad));
}

// ------------------------------------------------------------------------------------------
// Per CU: the whole LDS as memory, then a known-answer matrix chain on every SIMD
// ------------------------------------------------------------------------------------------

constexpr int CU_WAVES = 16;                       // per workgroup: four per SIMD when spread evenly
constexpr int CU_THREADS = CU_WAVES * 64;
constexpr int CU_LDS_BYTES = 163840;               // all of a CU's LDS: no second workgroup fits beside this one
constexpr int CU_LDS_WORDS = CU_LDS_BYTES / 4;     // 40960
constexpr int CU_LDS_CHUNKS = CU_LDS_BYTES / 16;   // 10240, ten per thread and sweep
constexpr int CU_K_CAP = 304;                      // 256 rows x (2 * 304 + 16) B = 159744 B <= 163840 B
constexpr int CU_PITCH = CU_K_CAP * 2 + 16;        // 624 B: an operand row and its pad
constexpr int CU_ROWS = 256;                       // four 32-row panels of A, then four of B
constexpr int CU_NOT_INT = INT32_MIN;              // the delta of an accumulator that holds no integer

// s_getreg operand: (size - 1) << 11 | offset << 6 | register.  Both are reads of status registers.
constexpr int CU_GETREG_HW_ID = (31 << 11) | 4;    // HW_REG_HW_ID, all 32 bits
constexpr int CU_GETREG_XCC_ID = (3 << 11) | 20;   // HW_REG_XCC_ID, bits 3:0

struct CuWave {  // what one wave saw; the host puts the sixteen of a workgroup together
  uint32_t hw_id, xcc_id;
  uint32_t lds_count, lds_offset, lds_expected, lds_got;  // mismatching words; one of them
  uint32_t mfma_count;                                    // mismatching accumulator elements; one of them
  int mfma_i, mfma_j, mfma_delta;
};
struct CuResult {
  CuWave wave[CU_WAVES];
};
struct CuArgs {
  uint32_t seed;
  int passes, K, reps;
  int flip_wg, flip_word;  // flip_wg, poison_wg < 0: none
  uint32_t flip_mask;
  int poison_wg, poison_wave, poison_i, poison_j;
};

// What pass `pass` leaves in LDS word `word` of workgroup `wg`: as hbm_pattern, a hash of the
// address, complemented on odd passes.
__host__ __device__ static inline uint32_t lds_pattern(uint32_t seed, uint32_t wg, uint32_t word, uint32_t pass) {
  const uint32_t h = mix32(seed ^ (mix32(wg + (pass >> 1) * 0x9e3779b9u) + word));
  return (pass & 1u) ? ~h : h;
}

// The integer side's view of an operand and of an accumulator: decoded from the bit pattern
// with integer operations, never a conversion (as f64_int above).  An operand is 0, +-1
// (exponent 127) or +-2 (128).
__device__ static inline int bf16_small_int(uint32_t bits16) {
  const int e = (bits16 >> 7) & 0xff, mag = e ? 1 << ((e - 127) & 31) : 0;
  return (bits16 & 0x8000u) ? -mag : mag;
}

// False when the float holds no integer of magnitude below 2^24: a fraction, an infinity, a NaN.
__device__ static inline bool f32_int(uint32_t bits, int* out) {
  const int e = (bits >> 23) & 0xff;
  const uint32_t frac = bits & 0x7fffffu;
  *out = 0;
  if (e == 0) return frac == 0;          // +-0; a subnormal is a fraction
  if (e < 127 || e > 150) return false;  // below 1; 2^24 and above, infinity, NaN
  const uint32_t sig = 0x800000u | frac;  // the value is sig * 2^(e - 150)
  const int drop = 150 - e;               // 0 .. 23
  if (sig & ((1u << drop) - 1u)) return false;
  const int mag = static_cast<int>(sig >> drop);
  *out = (bits >> 31) ? -mag : mag;
  return true;
}

// Compiled for gfx950 (-O3, kernel-resource-usage): 92 VGPRs + 0 AGPRs, 163840 B LDS, 0 scratch,
// 0 SGPR/VGPR spills; occupancy 4 waves per SIMD, which is this one workgroup: the LDS admits
// no second one on the CU.
//
// The work split is by hardware unit, not by data.  A workgroup declares all 160 KB of LDS, so
// it has a CU to itself, and the grid is one workgroup per CU of the device: on an idle device
// every CU gets one.  No workgroup waits for another.  Its 16 waves are more than the 4 SIMDs;
// each wave reads HW_REG_HW_ID and HW_REG_XCC_ID (s_getreg_b32, scalar reads of status
// registers) and reports what it read, so the host sees the CU (XCC, SE, SH, CU) and which
// SIMD each wave ran on.  HW_ID on this family: wave slot 3:0, SIMD 5:4, pipe 7:6, CU 11:8,
// SH 12, SE 14:13; XCC_ID 3:0.  The kernel hands the registers over whole; the host decodes.
//
// Phase A, LDS as memory: moving inversions over the 10240 16-byte chunks.  Sweep s checks what
// sweep s-1 wrote and stores pass s (odd passes the complement); sweep `passes` only checks.
// In sweep s thread t owns chunks 1024 i + ((t + 65 s) & 1023), i = 0..9: one ds_read_b128 and
// one ds_write_b128 each.  The 64 lanes of a wave touch 64 consecutive chunks (a run that wraps
// at 1024 keeps chunk mod 16 = (t + 65 s) mod 16), so any 16 lanes served together whose lane
// numbers are distinct mod 16 (16 consecutive ones, or the sets {0-3, 12-15, 20-23, 24-27} and
// {4-7, 8-11, 16-19, 28-31} of the FP64 kernel's comment) start in 16 distinct 4-bank groups of
// the 64 banks: conflict-free.  The step of 65 moves a chunk to the next wave (for most
// placements another SIMD) and the next lane each sweep, so no cell is always written and read
// through the same lane; a barrier separates the sweeps.
//
// Phase B, the matrix unit of each SIMD: the workgroup regenerates operands in the LDS it has
// just verified, integers in [-2, 2] as bf16 from the hash of the GEMM inputs: four 32 x K_CAP
// panels of A and four of B.  Wave w owns the 32x32 block (w / 4, w % 4): A panel w / 4 against
// B panel w % 4, sixteen different blocks from eight panels, which is what lets K reach 304 (a
// panel pair per wave would stop at 128).  The chain is K / 16 v_mfma_f32_32x32x16_bf16 into
// one accumulator, `reps` times from zero; lane l reads row (A) or column (B) l % 32 at k
// 8 * (l / 32) .. + 7 with one ds_read_b128 per operand and instruction.  Rows are *padded* to
// 624 bytes, 39 chunks: the 16 lanes served together read rows with 16 distinct r mod 16 (in
// either lane grouping above) at one k offset, chunk 39 r + c, and 39 is odd, so 39 r mod 16
// takes 16 distinct values: conflict-free.  Padding over a swizzle as in the bf16 GEMM: one
// multiply-add per address, and the integer side below reads the same rows without undoing an xor.
//
// The expected block comes from the same LDS operands in 32-bit integer VALU arithmetic: each
// lane forms the 16 dot products of its accumulator elements (register r of lane l is
// D[8 * (r / 4) + 4 * (l / 32) + r % 4][l % 32]) once, decoding bf16 by shifts, and after every
// chain decodes its 16 floats to integers by their bit patterns and compares with ==.  No
// floating-point instruction is on that side.  |a b| <= 4, so a partial sum is an integer of
// magnitude <= 4 K <= 1216, far below 2^24: fp32 holds it exactly in any order.
__global__ __launch_bounds__(CU_THREADS) void cu_check_kernel(CuResult* __restrict__ res, CuArgs a) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[CU_LDS_CHUNKS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t wg = blockIdx.x;
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(CU_GETREG_HW_ID);
  const uint32_t xcc_id = __builtin_amdgcn_s_getreg(CU_GETREG_XCC_ID);

  // ---- phase A
  uint32_t bad = 0, bad_word = 0, bad_want = 0, bad_got = 0;
  for (int s = 0; s <= a.passes; ++s) {
    const int slot = (t + 65 * s) & (CU_THREADS - 1);
    for (int i = 0; i < CU_LDS_CHUNKS / CU_THREADS; ++i) {
      const int c = i * CU_THREADS + slot;
      if (s > 0) {
        const u32x4 got = lds[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t want = lds_pattern(a.seed, wg, 4 * c + e, static_cast<uint32_t>(s - 1));
          if (got[e] != want) {
            if (bad == 0) bad_word = 4 * c + e, bad_want = want, bad_got = got[e];
            ++bad;
          }
        }
      }
      if (s < a.passes) {
        u32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = lds_pattern(a.seed, wg, 4 * c + e, static_cast<uint32_t>(s));
        lds[c] = v;
      }
    }
    __syncthreads();
    if (s == 0 && a.flip_wg == static_cast<int>(wg)) {  // detector self-test: one word changed between two sweeps
      if (t == 0 && a.flip_word >= 0 && a.flip_word < CU_LDS_WORDS)
        reinterpret_cast<uint32_t*>(lds)[a.flip_word] ^= a.flip_mask;
      __syncthreads();
    }
  }

  // ---- phase B: operands; row r of the 256 is row r % 32 of panel r / 32
  unsigned char* const base = reinterpret_cast<unsigned char*>(lds);
  const uint32_t gs = mix32(a.seed + wg * 0x9e3779b9u);
  for (int c = t; c < CU_ROWS * (CU_K_CAP / 8); c += CU_THREADS) {
    const uint32_t row = c / (CU_K_CAP / 8), col = c % (CU_K_CAP / 8) * 8;
    u32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      v[e] = small_int_bf16(gs, row, col + 2 * e) | (small_int_bf16(gs, row, col + 2 * e + 1) << 16);
    *reinterpret_cast<u32x4*>(base + row * CU_PITCH + col * 2) = v;
  }
  __syncthreads();  // from here LDS is only read

  const int wm = w >> 2, wn = w & 3, l32 = lane & 31, half = lane >> 5;
  const unsigned char* const pa = base + wm * 32 * CU_PITCH;                   // this wave's panel of A
  const unsigned char* const pb = base + (128 + wn * 32 + l32) * CU_PITCH;     // this lane's column of B
  int want[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) want[r] = 0;
  for (int c8 = 0; c8 < a.K / 8; ++c8) {
    const u32x4 bv = *reinterpret_cast<const u32x4*>(pb + c8 * 16);
    int b[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) b[2 * e] = bf16_small_int(bv[e] & 0xffffu), b[2 * e + 1] = bf16_small_int(bv[e] >> 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const u32x4 av = *reinterpret_cast<const u32x4*>(pa + (8 * (r >> 2) + 4 * half + (r & 3)) * CU_PITCH + c8 * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        want[r] += bf16_small_int(av[e] & 0xffffu) * b[2 * e] + bf16_small_int(av[e] >> 16) * b[2 * e + 1];
    }
  }

  const unsigned char* const sa = pa + l32 * CU_PITCH + half * 16;
  const unsigned char* const sb = pb + half * 16;
  const bool poison = a.poison_wg == static_cast<int>(wg) && a.poison_wave == w && a.poison_j == l32;
  uint32_t mbad = 0;
  int mbad_i = 0, mbad_delta = 0;
  for (int rep = 0; rep < a.reps; ++rep) {
    asm volatile("" ::: "memory");  // every chain reads its operands again
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int kk = 0; kk < a.K / 16; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(sa + kk * 32),
                                                    *reinterpret_cast<const bf16x8*>(sb + kk * 32), acc, 0, 0, 0);
    if (poison && rep == 0) {  // detector self-test: one element off by one
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += 8 * (r >> 2) + 4 * half + (r & 3) == a.poison_i ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int have;
      const bool whole = f32_int(__float_as_uint(acc[r]), &have);
      if (!whole || have != want[r]) {
        if (mbad == 0) mbad_i = 8 * (r >> 2) + 4 * half + (r & 3), mbad_delta = whole ? have - want[r] : CU_NOT_INT;
        ++mbad;
      }
    }
  }

  // ---- the wave's record: counts summed over the lanes, the details of its lowest lane that has any
  const unsigned long long lds_lanes = __ballot(bad != 0), mfma_lanes = __ballot(mbad != 0);
  const int lds_src = lds_lanes ? __ffsll(lds_lanes) - 1 : 0, mfma_src = mfma_lanes ? __ffsll(mfma_lanes) - 1 : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off), mbad += __shfl_xor(mbad, off);
  const CuWave rec = {hw_id,
                      xcc_id,
                      bad,
                      4u * __shfl(bad_word, lds_src),
                      __shfl(bad_want, lds_src),
                      __shfl(bad_got, lds_src),
                      mbad,
                      __shfl(mbad_i, mfma_src),
                      mfma_src & 31,
                      __shfl(mbad_delta, mfma_src)};
  if (lane == 0) res[wg].wave[w] = rec;
}

// ------------------------------------------------------------------------------------------
// Fused attention: S^T = K Q^T, base-2 online softmax, O'^T = V^T P^T
// ------------------------------------------------------------------------------------------

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AT_QROWS = 128;                // query rows per workgroup, 32 per wave
constexpr int AT_KEYS = 64;                  // keys per LDS stage
constexpr int AT_VPITCH = AT_KEYS * 2 + 16;  // a row of the transposed V tile: 64 keys and a pad
constexpr int AT_FRAC = 12;                  // every result is a multiple of 2^-12
constexpr int AT_S_CAP = 2048;               // 2 S 2^12 <= 2^24
constexpr float AT_M0 = -64.0f;              // where the running maximum starts: below every score (|s| <= 6)

// The Q inputs: row `row` holds +-1 at three hashed columns, summed where they collide, so the
// sum of magnitudes of a row is at most 3 by construction.  One thread writes 8 consecutive bf16.
__global__ __launch_bounds__(256) void generate_q_kernel(uint16_t* __restrict__ x, size_t rows, int D, uint32_t seed) {
  const size_t chunks = rows * (D / 8);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t c = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; c < chunks; c += stride) {
    const uint32_t row = static_cast<uint32_t>(c / (D / 8)), col = static_cast<uint32_t>(c % (D / 8)) * 8;
    const uint32_t hr = mix32(seed ^ (row * 0x9e3779b9u));
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      const uint32_t h = mix32(hr + k);
      const uint32_t at = (h >> 1) % static_cast<uint32_t>(D) - col;  // wraps to a large value when outside the chunk
#pragma unroll
      for (uint32_t e = 0; e < 8; ++e) v[e] += at == e ? ((h & 1u) ? -1 : 1) : 0;
    }
    u32x4 out;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int mag = v[e] < 0 ? -v[e] : v[e];  // 0, 1, 2, 3 -> 0, 1.0, 2.0, 1.5 * 2
      const uint32_t bits = (v[e] < 0 ? 0x8000u : 0u) | (mag == 0 ? 0u : mag == 1 ? 0x3f80u : mag == 2 ? 0x4000u : 0x4040u);
      if (e & 1) out[e / 2] |= bits << 16;
      else out[e / 2] = bits;
    }
    *reinterpret_cast<u32x4*>(x + c * 8) = out;
  }
}

// The softmax of one 64-key tile for this lane's query, on the 32 scores the lane holds, and the
// exchange with lane l ^ 32 that holds the other 32.  Updates the running maximum and sum and
// packs the probabilities as the four B operands of the O' step; returns the rescale factor.  MASK: entries with key > query
// get p = 0 and stay out of the maximum.
template <bool MASK>
__device__ __forceinline__ float attn_softmax(const f32x16 (&sc)[2], int lane_key, int qi, float& m_run, float& l_run,
                                             bf16x8 (&pf)[4]) {
  float m_new = m_run;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool on = !MASK || lane_key + 32 * kb + 8 * (r >> 2) + (r & 3) <= qi;
      m_new = on ? fmaxf(m_new, sc[kb][r]) : m_new;
    }
  m_new = fmaxf(m_new, __shfl_xor(m_new, 32));
  float psum = 0.0f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool on = !MASK || lane_key + 32 * kb + 8 * (r >> 2) + (r & 3) <= qi;
      const float p = on ? __builtin_amdgcn_exp2f(sc[kb][r] - m_new) : 0.0f;
      psum += p;
      pf[2 * kb + (r >> 3)][r & 7] = static_cast<__bf16>(p);
    }
  psum += __shfl_xor(psum, 32);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // the rescale factor, for O' as well
  l_run = l_run * alpha + psum;
  m_run = m_new;
  return alpha;
}

// Compiled for gfx950 (-O3, kernel-resource-usage):
//   d = 64:  129 VGPRs (causal 142) + 0 AGPRs, 36864 B LDS, 0 scratch, 0 SGPR/VGPR spills, occupancy 3
//   d = 128: 201 VGPRs (causal 208) + 0 AGPRs, 71680 B LDS, 0 scratch, 0 SGPR/VGPR spills, occupancy 2
// waves per SIMD.  The launch bounds ask for two workgroups per CU: left alone the compiler puts
// the O' accumulators into AGPRs (190 + 64, causal 199 + 64 at occupancy 1) and moves all 64 to
// VGPRs and back for every rescale.  At d = 128 a lane holds 64 registers of O', 32 of Q, 32 of
// scores, 16 of packed P and 32 of global loads in flight.
//
// One forward pass of flash attention per (query block, head): O'[i][c] = sum_j 2^(s[i][j] - m[i]) V[j][c]
// with s = Q K^T, m the row maximum and l the row sum of the powers; base 2, no 1/sqrt(d), no
// final division (see the header).  Its design is not that of the GEMMs.
//
// Work split.  The grid is (ceil(S / 128), H).  A workgroup has 4 waves and wave w owns the 32
// query rows from 128 * block + 32 w for the whole kernel; S is a multiple of 64, so the last
// block may have rows for two waves only, and the other two just help to copy and keep the
// barriers.  Tiles of 64 keys of K and V move through LDS, double buffered: the global loads of
// tile kt + 1 are in flight while tile kt is computed, and are stored after it.
//
// Transposed formulation.  The wave computes S^T = K Q^T with v_mfma_f32_32x32x16_bf16 (layout
// as in gemm_abft_kernel's comment): K rows are the A operand from LDS, the wave's 32 rows of Q
// the B operand, lane l holding Q[q0 + l % 32][16 t + 8 (l / 32) .. + 7] in d / 16 x 4 registers
// for the whole kernel.  Register r of the accumulator of key block kb (32 keys) then holds, in
// lane l, the score of ONE query, l % 32, for key 32 kb + 8 (r / 4) + 4 (l / 32) + r % 4: a lane
// has 32 scores of its query per tile, the lane l ^ 32 the other 32.  Row maximum and row sum are
// an in-lane reduction over those registers and one exchange with lane l ^ 32; m, l and the
// rescale factor 2^(m_old - m_new) are per lane, and rescaling O' is a multiply of the lane's own
// accumulators: O'^T = V^T P^T has the query in the column, l % 32, too.  Nothing is broadcast.
//
// P never leaves registers.  p = 2^(s - m) comes from v_exp_f32 (__builtin_amdgcn_exp2f), eight
// of them are packed to bf16 (v_cvt_pk_bf16_f32) and are the B operand of step u of O'^T: the
// registers 8 (u % 2) .. + 7 of key block u / 2.  As an operand they stand for k = 8 (l / 32) .. + 7,
// but hold the keys {16 u + 4 h + 0..3, 16 u + 8 + 4 h + 0..3}, h = l / 32.  A sum over k does
// not care which key sits at which k as long as both operands agree, so the A operand, V^T, is
// read for the same keys in the same order and nothing is shuffled between lanes.
//
// V reaches the matrix unit key-contiguous by being written transposed into LDS when the stage
// is stored: row c of the stage holds the 64 keys of column c, and key k of a 16-key group sits
// at position k with bits 2 and 3 swapped, so the eight keys a lane needs are 16 consecutive
// bytes, one ds_read_b128.  (Chosen over the transposing LDS loads of gfx950, ds_read_b64_tr_b16:
// their lane-to-element map would have been one more supposition to settle on the device, on the
// side of the comparison that has to be trusted; a transposed store is plain address arithmetic.
// It costs 8 ds_write_b32 per 2 keys x 8 columns where a straight copy has 2 ds_write_b128.)
// A thread takes two adjacent keys and 8 columns from global memory, pairs the two keys' values
// of a column in one word and writes 8 words, one per column row.
//
// LDS: per stage 64 rows of K, d bf16 + 16 B pad (144 or 272 B), and d rows of V^T, 64 keys +
// 16 B pad (144 B); two stages, 36 KB (d = 64) or 70 KB (d = 128).  Rows are padded, as in the
// bf16 GEMM.  The operand reads are one ds_read_b128 per lane, served 16 lanes at a time, either
// 16 consecutive lanes or the sets {0-3, 12-15, 20-23, 24-27}, {4-7, 8-11, 16-19, 28-31} (+ 32)
// of the FP64 kernel's comment: each set reads 16 rows with 16 distinct r mod 16 at one offset.
// With 64 banks of 4 bytes row r starts at bank 36 r mod 64 = 4 (9 r mod 16) (pitch 144) or
// 68 r mod 64 = 4 (r mod 16) (pitch 272): sixteen distinct 4-bank groups, conflict-free.  The
// K stage writes are whole 16-byte chunks, 8 or 16 lanes per row, as in the bf16 GEMM.  The V^T
// writes are ds_write_b32, 64 lanes at once: lane l of a wave writes key pair l % 32 (word
// position: a bijection of it) of column rows 8 cc + e, cc = 2 w + l / 32; the word address is
// 36 (8 cc + e) + position = 32 cc + 36 e + position mod 64, and two values of cc 32 apart with 32
// positions each cover every bank once: conflict-free.
//
// Causal.  Key tiles wholly above the diagonal of the query block are not visited (the block
// stops after tile 2 * block + 1), and a wave skips a tile that is wholly above its own 32 rows.
// In a tile that the diagonal crosses, an entry with key > query gets p = 0 and its score is
// kept out of the running maximum.  Tile 0 holds key 0, which no row masks, so after tile 0
// every row has a true maximum.
//
// The running maximum starts at -64, below every score, so the first tile is no special case:
// its m_new is the tile's own maximum, at least -6, the rescale factor is 2^(-64 - m_new), a
// normal fp32 between 2^-70 and 2^-58, and l and O' are +0: 0 x a finite factor is exactly 0.
//
// Every key tile lies inside S (a multiple of 64), and Q rows and the stores are guarded by the
// wave's `live`, so no address outside the three inputs and two outputs is formed.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K,
                                                   const uint16_t* __restrict__ V, int S, float* __restrict__ O,
                                                   float* __restrict__ ML, int poison_h, int poison_i, int poison_c) {
  constexpr int KP = 2 * D + 16;                                  // pitch of a K row in LDS
  constexpr int K_BYTES = AT_KEYS * KP, STAGE = K_BYTES + D * AT_VPITCH;
  constexpr int CPR = D / 8, RPS = 256 / CPR, KQ = AT_KEYS / RPS;  // K copy: chunks per row, rows per sweep, sweeps
  constexpr int VI = D / 64;                                       // V copy: (key pair, 8 columns) items per thread
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];  // [stage][K, V^T]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l32 = lane & 31, half = lane >> 5;
  // causal blocks differ in length, 2 to S / 64 tiles: the long ones are dispatched first
  const int qb = CAUSAL ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int head = blockIdx.y, q0 = qb * AT_QROWS + w * 32, qi = q0 + l32;  // the wave's first query, the lane's
  const size_t hbase = static_cast<size_t>(head) * S;  // rows before this head
  const bool live = q0 < S;
  const int ntiles = CAUSAL ? min(S / AT_KEYS, 2 * qb + 2) : S / AT_KEYS;

  const u32x4 zero = {0u, 0u, 0u, 0u};
  bf16x8 qf[D / 16];
#pragma unroll
  for (int tt = 0; tt < D / 16; ++tt)
    qf[tt] = __builtin_bit_cast(bf16x8, live ? *reinterpret_cast<const u32x4*>(Q + (hbase + qi) * D + tt * 16 + half * 8) : zero);

  const int lr = t / CPR, kc = t % CPR;
  u32x4 gk[KQ], gv[VI][2];
#define LOAD_GLOBAL(tile)                                                                      \
  do {                                                                                         \
    const size_t r0_ = hbase + static_cast<size_t>(tile) * AT_KEYS;                            \
    _Pragma("unroll") for (int q = 0; q < KQ; ++q)                                             \
      gk[q] = *reinterpret_cast<const u32x4*>(K + (r0_ + lr + RPS * q) * D + kc * 8);          \
    _Pragma("unroll") for (int i = 0; i < VI; ++i) {                                           \
      const int x_ = t + 256 * i, pr_ = x_ & 31, cc_ = x_ >> 5;                                \
      gv[i][0] = *reinterpret_cast<const u32x4*>(V + (r0_ + 2 * pr_) * D + cc_ * 8);           \
      gv[i][1] = *reinterpret_cast<const u32x4*>(V + (r0_ + 2 * pr_ + 1) * D + cc_ * 8);       \
    }                                                                                          \
  } while (0)
#define STORE_LDS(stage)                                                                       \
  do {                                                                                         \
    unsigned char* sk_ = lds + (stage) * STAGE + lr * KP + kc * 16;                            \
    _Pragma("unroll") for (int q = 0; q < KQ; ++q) *reinterpret_cast<u32x4*>(sk_ + RPS * q * KP) = gk[q]; \
    _Pragma("unroll") for (int i = 0; i < VI; ++i) {                                           \
      const int x_ = t + 256 * i, key_ = 2 * (x_ & 31), cc_ = x_ >> 5;                         \
      const int pos_ = (key_ & ~12) | ((key_ & 4) << 1) | ((key_ & 8) >> 1);                   \
      unsigned char* sv_ = lds + (stage) * STAGE + K_BYTES + cc_ * 8 * AT_VPITCH + pos_ * 2;   \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                          \
        const uint32_t a_ = gv[i][0][j], b_ = gv[i][1][j];                                     \
        *reinterpret_cast<uint32_t*>(sv_ + (2 * j) * AT_VPITCH) = (a_ & 0xffffu) | (b_ << 16); \
        *reinterpret_cast<uint32_t*>(sv_ + (2 * j + 1) * AT_VPITCH) = (a_ >> 16) | (b_ & 0xffff0000u); \
      }                                                                                        \
    }                                                                                          \
  } while (0)

  f32x16 acc[D / 32];  // O'^T: block cb holds columns 32 cb .. + 31 of the wave's 32 queries
#pragma unroll
  for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
  float m_run = AT_M0, l_run = 0.0f;

  LOAD_GLOBAL(0);
  STORE_LDS(0);
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const int stage = kt & 1, key0 = kt * AT_KEYS;
    const bool more = kt + 1 < ntiles;
    if (more) LOAD_GLOBAL(kt + 1);  // in flight while this tile is computed
    if (live && !(CAUSAL && key0 > q0 + 31)) {
      const unsigned char* sk = lds + stage * STAGE + l32 * KP + half * 16;
      f32x16 sc[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[kb][r] = 0.0f;
#pragma unroll
        for (int tt = 0; tt < D / 16; ++tt)
          sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(sk + kb * 32 * KP + tt * 32),
                                                           qf[tt], sc[kb], 0, 0, 0);
      }
      // the diagonal crosses this tile for some row of the wave: only then is an entry compared with its row
      const bool diag = CAUSAL && key0 + AT_KEYS - 1 > q0;
      const int lane_key = key0 + 4 * half;  // entry (kb, r) is key lane_key + 32 kb + 8 (r / 4) + r % 4
      bf16x8 pf[4];
      const float alpha = diag ? attn_softmax<true>(sc, lane_key, qi, m_run, l_run, pf)
                               : attn_softmax<false>(sc, lane_key, qi, m_run, l_run, pf);
#pragma unroll
      for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] *= alpha;
      const unsigned char* sv = lds + stage * STAGE + K_BYTES + l32 * AT_VPITCH + half * 16;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int cb = 0; cb < D / 32; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(sv + cb * 32 * AT_VPITCH + u * 32),
                                                           pf[u], acc[cb], 0, 0, 0);
    }
    // the other stage was last read in tile kt-1, before the barrier that ended it
    if (more) STORE_LDS(stage ^ 1);
    __syncthreads();
  }
#undef LOAD_GLOBAL
#undef STORE_LDS

  if (!live) return;  // past the last barrier
  // register r of block cb is O'[qi][32 cb + 8 (r / 4) + 4 half + r % 4]: four consecutive columns per r / 4
  if (poison_h == head && poison_i == qi) {  // detector self-test: one element off by one unit
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[cb][r] += 32 * cb + 8 * (r >> 2) + 4 * half + (r & 3) == poison_c ? 0x1p-12f : 0.0f;
  }
  float* const orow = O + (hbase + qi) * D + 4 * half;
#pragma unroll
  for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = {acc[cb][4 * g], acc[cb][4 * g + 1], acc[cb][4 * g + 2], acc[cb][4 * g + 3]};
      *reinterpret_cast<f32x4*>(orow + 32 * cb + 8 * g) = v;
    }
  if (half == 0) {
    const f32x2 ml = {m_run, l_run};
    *reinterpret_cast<f32x2*>(ML + (hbase + qi) * 2) = ml;
  }
}

// The expected side, in integers: nothing below is shared with attn_kernel and no floating-point
// instruction is on it.  A Q element is an integer of magnitude < 256 in bf16 (here at most 3),
// decoded by shifts; false for a fraction, an infinity, a NaN.
__host__ __device__ static inline bool bf16_whole(uint32_t bits16, int* out) {
  const int e = (bits16 >> 7) & 0xff, frac = bits16 & 0x7f;
  *out = 0;
  if (e == 0) return frac == 0;          // +-0; a subnormal is a fraction
  if (e < 127 || e > 134) return false;  // below 1; 256 and above, infinity, NaN
  const int sig = 0x80 | frac, drop = 134 - e;  // the value is sig * 2^(e - 134)
  if (sig & ((1 << drop) - 1)) return false;
  *out = (bits16 & 0x8000u) ? -(sig >> drop) : sig >> drop;
  return true;
}

// One workgroup per (row i, head), in units of 2^-12: ofix[i][c] = sum_j V[j][c] << (s_j - m + 12),
// mlfix[i] = {m << 12, sum_j 1 << (s_j - m + 12)}, over j <= i when causal.  Two passes over the
// keys: the scores and their maximum, then the sums.  s_j - m + 12 is in [0, 12], |ofix| <= 2 S 2^12.
__global__ __launch_bounds__(256) void expect_attn_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K,
                                                          const uint16_t* __restrict__ V, int S, int D, int causal,
                                                          int* __restrict__ ofix, int* __restrict__ mlfix) {
  __shared__ int qrow[128], score[AT_S_CAP], red[256];
  const int t = threadIdx.x, i = blockIdx.x;
  const size_t hbase = static_cast<size_t>(blockIdx.y) * S;
  const int n = causal ? i + 1 : S;
  if (t < D) bf16_whole(Q[(hbase + i) * D + t], &qrow[t]);
  __syncthreads();
  int mx = INT32_MIN;
  for (int j = t; j < n; j += 256) {
    const uint16_t* kr = K + (hbase + j) * D;
    int s = 0;
    for (int c = 0; c < D; c += 8) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(kr + c);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        s += qrow[c + 2 * e] * bf16_small_int(v[e] & 0xffffu) + qrow[c + 2 * e + 1] * bf16_small_int(v[e] >> 16);
    }
    score[j] = s;
    mx = max(mx, s);
  }
  red[t] = mx;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (t < off) red[t] = max(red[t], red[t + off]);
    __syncthreads();
  }
  const int m = red[0];
  __syncthreads();
  int lsum = 0;
  for (int j = t; j < n; j += 256) lsum += 1 << (score[j] - m + AT_FRAC);
  red[t] = lsum;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) {
    mlfix[(hbase + i) * 2] = m * (1 << AT_FRAC);
    mlfix[(hbase + i) * 2 + 1] = red[0];
  }
  __syncthreads();
  // thread t adds column t % D over the keys of slice t / D, then the 256 / D slices are added
  const int c = t % D, slices = 256 / D;
  int o = 0;
  for (int j = t / D; j < n; j += slices) o += bf16_small_int(V[(hbase + j) * D + c]) * (1 << (score[j] - m + AT_FRAC));
  red[t] = o;
  __syncthreads();
  if (t < D) {
    int sum = 0;
    for (int sl = 0; sl < slices; ++sl) sum += red[sl * D + t];
    ofix[(hbase + i) * D + t] = sum;
  }
}

// f32_int with an exponent offset: the float times 2^frac_bits as an integer, by bit pattern.
// False when it is no such multiple of magnitude below 2^31: a finer fraction, an infinity, a NaN.
__device__ static inline bool f32_fixed(uint32_t bits, int frac_bits, int* out) {
  const int e = (bits >> 23) & 0xff;
  const uint32_t frac = bits & 0x7fffffu;
  *out = 0;
  if (e == 0) return frac == 0;            // +-0; a subnormal is a fraction
  const int up = e - 150 + frac_bits;       // the scaled value is sig * 2^up
  if (up > 7 || up < -23) return false;     // 2^31 and above, infinity, NaN; below one unit
  const uint32_t sig = 0x800000u | frac;
  if (up < 0 && (sig & ((1u << -up) - 1u))) return false;
  const int mag = static_cast<int>(up < 0 ? sig >> -up : sig << up);
  *out = (bits >> 31) ? -mag : mag;
  return true;
}

struct AttnRecord {
  int kind;  // 0 "o", 1 "l", 2 "m"
  int head, i, c, delta;
};
struct AttnResult {
  unsigned int count, no, nml;
  AttnRecord o[MAX_RECORDS], ml[MAX_RECORDS];  // the first few wrong O' elements, the first few wrong l or m
};

// Every fp32 of O' (H S d of them) and of ML (H S pairs m, l) against its integer in units of
// 2^-12, with ==.  The delta of a record is in those units, CU_NOT_INT for a value that is no
// multiple of the unit.
__global__ __launch_bounds__(256) void verify_attn_kernel(const float* __restrict__ O, const int* __restrict__ ofix,
                                                          const float* __restrict__ ML, const int* __restrict__ mlfix,
                                                          size_t no, size_t nml, int S, int D, AttnResult* res) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t x = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; x < no + nml; x += stride) {
    const bool is_o = x < no;
    const size_t y = is_o ? x : x - no;
    const int want = is_o ? ofix[y] : mlfix[y];
    int have;
    const bool whole = f32_fixed(__float_as_uint(is_o ? O[y] : ML[y]), AT_FRAC, &have);
    if (whole && have == want) continue;
    atomicAdd(&res->count, 1u);
    const unsigned int slot = atomicAdd(is_o ? &res->no : &res->nml, 1u);
    if (slot < MAX_RECORDS) {
      const size_t row = is_o ? y / D : y / 2;
      const AttnRecord rec = {is_o ? 0 : (y & 1) ? 1 : 2, static_cast<int>(row / S), static_cast<int>(row % S),
                              is_o ? static_cast<int>(y % D) : 0, whole ? have - want : CU_NOT_INT};
      (is_o ? res->o : res->ml)[slot] = rec;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------

static int grid_for(int dev) {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, dev));
  return prop.multiProcessorCount * 8;
}

static int usage(const char* why) {
  fprintf(stderr,
          "%s\nusage: gpu_check gemm [--dtype bf16|mxfp8|mxfp4|fp64|int8] --m M --n N --k K [--seed S] "
          "[--a FILE --b FILE [--sa FILE --sb FILE]] [--c-out FILE] [--poison I,J] "
          "[--device D] [--seconds T]\n         fp64: M and N multiples of 16, K a multiple of 4 and at most 8192; --a/--b "
          "hold doubles, integers of magnitude <= 65535\n         int8: M and N multiples of 32, K a multiple of 32 and at most "
          "65536; --a/--b hold raw int8 bytes, every value valid\n       gpu_check hbm --mib SIZE [--passes P] [--seed S] [--flip WORD:MASK] "
          "[--device D]\n       gpu_check cu [--k K] [--reps R] [--passes P] [--rounds N] [--seed S] [--flip WG:WORD:MASK] "
          "[--poison WG:WAVE:I,J] [--device D]\n         K a multiple of 16 and at most 304, what 16 waves' operands take of "
          "the 160 KB of LDS; WORD below 40960, WAVE below 16, I,J inside 32x32\n       gpu_check attn [--heads H] [--seq S] "
          "[--d 64|128] [--causal] [--seed S] [--seconds T] [--q FILE --k FILE --v FILE] [--o-out FILE] [--ml-out FILE] "
          "[--poison H,I,C] [--device D]\n         defaults: 64 heads, S 2048, d 128, not causal; S a multiple of 64 and at most "
          "2048; K and V hold integers in [-2, 2], every Q row integers with sum |q| <= 3\n",
          why);
  return 2;
}

// rows x K raw little-endian bf16 from a file; every value must be an integer in [-2, 2]
static bool read_operand(const std::string& path, size_t elems, std::vector<uint16_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out->resize(elems);
  const size_t got = fread(out->data(), 2, elems, f);
  const bool exact = got == elems && fgetc(f) == EOF;
  fclose(f);
  if (!exact) return false;
  for (uint16_t b : *out)
    if (b != 0x0000 && b != 0x8000 && b != 0x3f80 && b != 0xbf80 && b != 0x4000 && b != 0xc000) return false;
  return true;
}

// exactly `bytes` raw bytes of a microscaling operand; `kind` is MXFP8 (E4M3 bytes of -2 .. 2),
// MXFP4 (two E2M1 codes of magnitude 0 .. 4 per byte, no negative zero), 0 (scales: 127, 128) or
// INT8 (every byte is valid: only the size is checked)
static bool read_mx(const std::string& path, size_t bytes, int kind, std::vector<unsigned char>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out->resize(bytes);
  const size_t got = fread(out->data(), 1, bytes, f);
  const bool exact = got == bytes && fgetc(f) == EOF;
  fclose(f);
  if (!exact) return false;
  const auto fp4 = [](unsigned c) { return (c & 7u) <= 4u && c != 8u; };
  for (unsigned char b : *out) {
    const bool good = kind == MXFP8   ? (b == 0x00 || b == 0x38 || b == 0x40 || b == 0xb8 || b == 0xc0)
                      : kind == MXFP4 ? (fp4(b & 15u) && fp4(b >> 4))
                      : kind == INT8  ? true
                                      : (b == 127 || b == 128);
    if (!good) return false;
  }
  return true;
}

// exactly `elems` little-endian doubles, each an integer of magnitude <= 65535 (-0 is one)
static bool read_f64(const std::string& path, size_t elems, std::vector<uint64_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out->resize(elems);
  const size_t got = fread(out->data(), 8, elems, f);
  const bool exact = got == elems && fgetc(f) == EOF;
  fclose(f);
  if (!exact) return false;
  for (uint64_t b : *out) {
    long long v;
    if (!f64_int(b, &v) || v < -65535 || v > 65535) return false;
  }
  return true;
}

struct GemmBuffers {
  unsigned char *A, *B, *SA, *SB;  // the scales only for the microscaling formats
  float *colsum, *rowsum, *C;      // doubles for FP64; int64 sums and an int32 C for INT8
  int *ea, *eb, *colexp, *rowexp;  // colexp, rowexp: int64 for FP64 and INT8
};

// One pass: fresh inputs when asked, the GEMM between the two events, the expected checksums.
template <int FMT>
static void gemm_pass(const GemmBuffers& g, int M, int N, int K, int grid, bool generate, uint32_t s, int poison_i,
                      int poison_j, hipEvent_t ev0, hipEvent_t ev1) {
  const int tiles_m = (M + TILE - 1) / TILE, tiles_n = (N + TILE - 1) / TILE;
  const dim3 tiles(tiles_n, tiles_m), b256(256), kx_m((K + 255) / 256, tiles_m), kx_n((K + 255) / 256, tiles_n);
  const dim3 ex_col(N, (tiles_m + 3) / 4), ex_row(M, (tiles_n + 3) / 4);
  if constexpr (FMT == BF16) {
    uint16_t *A = reinterpret_cast<uint16_t*>(g.A), *B = reinterpret_cast<uint16_t*>(g.B);
    if (generate) {
      hipLaunchKernelGGL(generate_kernel, dim3(grid), b256, 0, 0, A, M, K, mix32(2 * s));
      hipLaunchKernelGGL(generate_kernel, dim3(grid), b256, 0, 0, B, N, K, mix32(2 * s + 1));
    }
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(gemm_abft_kernel, tiles, b256, 0, 0, A, B, M, N, K, g.colsum, g.rowsum, g.C, poison_i, poison_j);
    CHECK(hipEventRecord(ev1));
    hipLaunchKernelGGL(stripe_sum_kernel, kx_m, b256, 0, 0, A, M, K, g.ea);
    hipLaunchKernelGGL(stripe_sum_kernel, kx_n, b256, 0, 0, B, N, K, g.eb);
    hipLaunchKernelGGL(expect_kernel, ex_col, b256, 0, 0, g.ea, tiles_m, B, N, K, g.colexp);
    hipLaunchKernelGGL(expect_kernel, ex_row, b256, 0, 0, g.eb, tiles_n, A, M, K, g.rowexp);
  } else if constexpr (FMT == FP64) {
    uint64_t *A = reinterpret_cast<uint64_t*>(g.A), *B = reinterpret_cast<uint64_t*>(g.B);
    long long *colexp = reinterpret_cast<long long*>(g.colexp), *rowexp = reinterpret_cast<long long*>(g.rowexp);
    if (generate) {
      hipLaunchKernelGGL(generate_f64_kernel, dim3(grid), b256, 0, 0, A, M, K, mix32(2 * s));
      hipLaunchKernelGGL(generate_f64_kernel, dim3(grid), b256, 0, 0, B, N, K, mix32(2 * s + 1));
    }
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(gemm_abft_f64_kernel, tiles, b256, 0, 0, reinterpret_cast<const double*>(A),
                       reinterpret_cast<const double*>(B), M, N, K, reinterpret_cast<double*>(g.colsum),
                       reinterpret_cast<double*>(g.rowsum), reinterpret_cast<double*>(g.C), poison_i, poison_j);
    CHECK(hipEventRecord(ev1));
    hipLaunchKernelGGL(stripe_sum_f64_kernel, kx_m, b256, 0, 0, A, M, K, g.ea);
    hipLaunchKernelGGL(stripe_sum_f64_kernel, kx_n, b256, 0, 0, B, N, K, g.eb);
    hipLaunchKernelGGL(expect_f64_kernel, ex_col, b256, 0, 0, g.ea, tiles_m, B, N, K, colexp);
    hipLaunchKernelGGL(expect_f64_kernel, ex_row, b256, 0, 0, g.eb, tiles_n, A, M, K, rowexp);
  } else if constexpr (FMT == INT8) {
    long long *colexp = reinterpret_cast<long long*>(g.colexp), *rowexp = reinterpret_cast<long long*>(g.rowexp);
    const dim3 wg_tiles((N + I8_TILE_N - 1) / I8_TILE_N, tiles_m);  // 128 x 256 of C each; the stripes stay 128 wide
    const dim3 k4_m((K / 4 + 255) / 256, tiles_m), k4_n((K / 4 + 255) / 256, tiles_n);
    if (generate) {
      hipLaunchKernelGGL(generate_i8_kernel, dim3(grid), b256, 0, 0, g.A, M, K, mix32(2 * s));
      hipLaunchKernelGGL(generate_i8_kernel, dim3(grid), b256, 0, 0, g.B, N, K, mix32(2 * s + 1));
    }
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(gemm_abft_i8_kernel, wg_tiles, b256, 0, 0, g.A, g.B, M, N, K, reinterpret_cast<long long*>(g.colsum),
                       reinterpret_cast<long long*>(g.rowsum), reinterpret_cast<int*>(g.C), poison_i, poison_j);
    CHECK(hipEventRecord(ev1));
    hipLaunchKernelGGL(stripe_sum_i8_kernel, k4_m, b256, 0, 0, g.A, M, K, g.ea);
    hipLaunchKernelGGL(stripe_sum_i8_kernel, k4_n, b256, 0, 0, g.B, N, K, g.eb);
    hipLaunchKernelGGL(expect_i8_kernel, ex_col, b256, 0, 0, g.ea, tiles_m, g.B, N, K, colexp);
    hipLaunchKernelGGL(expect_i8_kernel, ex_row, b256, 0, 0, g.eb, tiles_n, g.A, M, K, rowexp);
  } else {
    if (generate) {
      hipLaunchKernelGGL(generate_mx_kernel<FMT>, dim3(grid), b256, 0, 0, g.A, M, K, mix32(2 * s));
      hipLaunchKernelGGL(generate_mx_kernel<FMT>, dim3(grid), b256, 0, 0, g.B, N, K, mix32(2 * s + 1));
      hipLaunchKernelGGL(generate_scale_kernel, dim3(grid), b256, 0, 0, g.SA, M, K / 32, mix32(2 * s));
      hipLaunchKernelGGL(generate_scale_kernel, dim3(grid), b256, 0, 0, g.SB, N, K / 32, mix32(2 * s + 1));
    }
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(gemm_abft_mx_kernel<FMT>, tiles, b256, 0, 0, g.A, g.B, g.SA, g.SB, M, N, K, g.colsum, g.rowsum,
                       g.C, poison_i, poison_j);
    CHECK(hipEventRecord(ev1));
    hipLaunchKernelGGL(stripe_sum_mx_kernel<FMT>, kx_m, b256, 0, 0, g.A, g.SA, M, K, g.ea);
    hipLaunchKernelGGL(stripe_sum_mx_kernel<FMT>, kx_n, b256, 0, 0, g.B, g.SB, N, K, g.eb);
    hipLaunchKernelGGL(expect_mx_kernel<FMT>, ex_col, b256, 0, 0, g.ea, tiles_m, g.B, g.SB, N, K, g.colexp);
    hipLaunchKernelGGL(expect_mx_kernel<FMT>, ex_row, b256, 0, 0, g.eb, tiles_n, g.A, g.SA, M, K, g.rowexp);
  }
}

static int run_gemm(int fmt, int M, int N, int K, uint32_t seed, const std::string& a_file, const std::string& b_file,
                    const std::string& sa_file, const std::string& sb_file, const std::string& c_out, int poison_i,
                    int poison_j, int device, double seconds) {
  if (fmt == BF16 && (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 16 || K > 32768))
    return usage("gemm: M and N must be multiples of 32, K a multiple of 16 and at most 32768");
  // the caps of the exactness argument in the header: 16*K*128 and 64*K*128 quarter-units <= 2^24
  const bool mx = fmt == MXFP8 || fmt == MXFP4;
  if (mx && (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 64 || K > (fmt == MXFP8 ? 8192 : 2048)))
    return usage("gemm: M and N must be multiples of 32, K a multiple of 64 and at most 8192 (mxfp8) or 2048 (mxfp4)");
  // 2^32 * K * 128 <= 2^52
  if (fmt == FP64 && (M <= 0 || N <= 0 || K <= 0 || M % 16 || N % 16 || K % 4 || K > 8192))
    return usage("gemm: M and N must be multiples of 16, K a multiple of 4 and at most 8192 (fp64)");
  // 2^14 * K <= 2^30: every element of C is inside int32
  if (fmt == INT8 && (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 32 || K > 65536))
    return usage("gemm: M and N must be multiples of 32, K a multiple of 32 and at most 65536 (int8)");
  if (a_file.empty() != b_file.empty()) return usage("gemm: --a and --b go together");
  if (!mx ? !(sa_file.empty() && sb_file.empty())
          : (sa_file.empty() != a_file.empty() || sb_file.empty() != a_file.empty()))
    return usage("gemm: --sa and --sb go with --a and --b, for the mx types only");
  if (poison_i >= M || poison_j >= N) return usage("gemm: --poison outside C");
  const size_t a_elems = static_cast<size_t>(M) * K, b_elems = static_cast<size_t>(N) * K;
  const size_t a_bytes = fmt == FP64 ? a_elems * 8 : fmt == BF16 ? a_elems * 2 : fmt == MXFP4 ? a_elems / 2 : a_elems;
  const size_t b_bytes = fmt == FP64 ? b_elems * 8 : fmt == BF16 ? b_elems * 2 : fmt == MXFP4 ? b_elems / 2 : b_elems;
  const size_t sum_size = fmt == FP64 || fmt == INT8 ? 8 : 4;  // of a checksum and an expectation
  const size_t c_size = fmt == FP64 ? 8 : 4;                    // of an element of C
  std::vector<uint16_t> ha, hb;
  std::vector<uint64_t> da, db;
  if (fmt == FP64 && !a_file.empty() && !(read_f64(a_file, a_elems, &da) && read_f64(b_file, b_elems, &db)))
    return usage("gemm: --a/--b must hold exactly M*K and N*K doubles, integers of magnitude <= 65535");
  std::vector<unsigned char> xa, xb, hsa, hsb;
  if (fmt == INT8 && !a_file.empty() && !(read_mx(a_file, a_bytes, INT8, &xa) && read_mx(b_file, b_bytes, INT8, &xb)))
    return usage("gemm: --a/--b must hold exactly M*K and N*K bytes (int8)");
  if (fmt == BF16 && !a_file.empty() && !(read_operand(a_file, a_elems, &ha) && read_operand(b_file, b_elems, &hb)))
    return usage("gemm: --a/--b must hold exactly M*K and N*K bf16 integers in [-2, 2]");
  if (mx && !a_file.empty() &&
      !(read_mx(a_file, a_bytes, fmt, &xa) && read_mx(b_file, b_bytes, fmt, &xb) &&
        read_mx(sa_file, a_elems / 32, 0, &hsa) && read_mx(sb_file, b_elems / 32, 0, &hsb)))
    return usage("gemm: --a/--b must hold exactly M*K and N*K E4M3 bytes of -2 .. 2 (mxfp8) or E2M1 codes of 0 .. 2 "
                 "in halves (mxfp4), --sa/--sb M*K/32 and N*K/32 bytes of 127 or 128");

  CHECK(hipSetDevice(device));
  const int grid = grid_for(device);
  const int tiles_m = (M + TILE - 1) / TILE, tiles_n = (N + TILE - 1) / TILE;
  const size_t ncol = static_cast<size_t>(tiles_m) * N, nrow = static_cast<size_t>(tiles_n) * M;
  GemmBuffers g = {};
  GemmResult* res = nullptr;
  CHECK(hipMalloc(&g.A, a_bytes));
  CHECK(hipMalloc(&g.B, b_bytes));
  if (mx) {
    CHECK(hipMalloc(&g.SA, a_elems / 32));
    CHECK(hipMalloc(&g.SB, b_elems / 32));
  }
  CHECK(hipMalloc(&g.colsum, ncol * sum_size));
  CHECK(hipMalloc(&g.rowsum, nrow * sum_size));
  CHECK(hipMalloc(&g.colexp, ncol * sum_size));
  CHECK(hipMalloc(&g.rowexp, nrow * sum_size));
  CHECK(hipMalloc(&g.ea, static_cast<size_t>(tiles_m) * K * 4));
  CHECK(hipMalloc(&g.eb, static_cast<size_t>(tiles_n) * K * 4));
  CHECK(hipMalloc(&res, sizeof(GemmResult)));
  if (!c_out.empty()) CHECK(hipMalloc(&g.C, static_cast<size_t>(M) * N * c_size));
  if (!a_file.empty()) {
    const void* pa = fmt == FP64 ? static_cast<const void*>(da.data()) : fmt == BF16 ? static_cast<const void*>(ha.data()) : xa.data();
    const void* pb = fmt == FP64 ? static_cast<const void*>(db.data()) : fmt == BF16 ? static_cast<const void*>(hb.data()) : xb.data();
    CHECK(hipMemcpy(g.A, pa, a_bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(g.B, pb, b_bytes, hipMemcpyHostToDevice));
    if (mx) {
      CHECK(hipMemcpy(g.SA, hsa.data(), hsa.size(), hipMemcpyHostToDevice));
      CHECK(hipMemcpy(g.SB, hsb.data(), hsb.size(), hipMemcpyHostToDevice));
    }
  }
  hipEvent_t ev0, ev1;
  CHECK(hipEventCreate(&ev0));
  CHECK(hipEventCreate(&ev1));

  GemmResult host = {};
  int passes = 0;
  double gemm_ms = 0.0;
  float* const C = g.C;
  const auto t0 = std::chrono::steady_clock::now();
  do {
    const uint32_t s = seed + static_cast<uint32_t>(passes);
    CHECK(hipMemset(res, 0, sizeof(GemmResult)));
    if (fmt == BF16) gemm_pass<BF16>(g, M, N, K, grid, a_file.empty(), s, poison_i, poison_j, ev0, ev1);
    else if (fmt == MXFP8) gemm_pass<MXFP8>(g, M, N, K, grid, a_file.empty(), s, poison_i, poison_j, ev0, ev1);
    else if (fmt == MXFP4) gemm_pass<MXFP4>(g, M, N, K, grid, a_file.empty(), s, poison_i, poison_j, ev0, ev1);
    else if (fmt == FP64) gemm_pass<FP64>(g, M, N, K, grid, a_file.empty(), s, poison_i, poison_j, ev0, ev1);
    else gemm_pass<INT8>(g, M, N, K, grid, a_file.empty(), s, poison_i, poison_j, ev0, ev1);
    if (fmt == INT8)
      hipLaunchKernelGGL(verify_i64_kernel, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const long long*>(g.colsum),
                         reinterpret_cast<const long long*>(g.colexp), ncol, N, reinterpret_cast<const long long*>(g.rowsum),
                         reinterpret_cast<const long long*>(g.rowexp), nrow, M, res);
    else if (fmt == FP64)
      hipLaunchKernelGGL(verify_f64_kernel, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const double*>(g.colsum),
                         reinterpret_cast<const long long*>(g.colexp), ncol, N, reinterpret_cast<const double*>(g.rowsum),
                         reinterpret_cast<const long long*>(g.rowexp), nrow, M, res);
    else  // the mxfp4 checksums are compared in quarter-units
      hipLaunchKernelGGL(verify_kernel, dim3(grid), dim3(256), 0, 0, g.colsum, g.colexp, ncol, N, g.rowsum, g.rowexp, nrow,
                         M, fmt == MXFP4 ? 4.0f : 1.0f, res);
    hipLaunchKernelGGL(locate_kernel, dim3(1), dim3(1), 0, 0, res, tiles_n);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(&host, res, sizeof(GemmResult), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    gemm_ms += ms;
    ++passes;
  } while (host.count == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);

  if (C != nullptr) {
    std::vector<unsigned char> hc(static_cast<size_t>(M) * N * c_size);  // floats, doubles for fp64, int32 for int8
    CHECK(hipMemcpy(hc.data(), C, hc.size(), hipMemcpyDeviceToHost));
    FILE* f = fopen(c_out.c_str(), "wb");
    if (!f || fwrite(hc.data(), 1, hc.size(), f) != hc.size()) return usage("gemm: cannot write --c-out");
    fclose(f);
  }
  const bool ok = host.count == 0;
  std::string recs;
  for (unsigned int r = 0; r < host.nrec; ++r) {
    const GemmRecord& g = host.rec[r];
    char buf[160];
    if (g.kind == 0)
      snprintf(buf, sizeof buf, "{\"kind\":\"element\",\"i\":%d,\"j\":%d,\"delta\":%g,\"tile\":%d}", g.i, g.j, g.delta, g.tile);
    else if (g.kind == 1)
      snprintf(buf, sizeof buf, "{\"kind\":\"row\",\"i\":%d,\"stripe\":%d,\"delta\":%g,\"tile\":%d}", g.i, g.j, g.delta, g.tile);
    else
      snprintf(buf, sizeof buf, "{\"kind\":\"column\",\"stripe\":%d,\"j\":%d,\"delta\":%g,\"tile\":%d}", g.i, g.j, g.delta, g.tile);
    recs += (r ? "," : "") + std::string(buf);
  }
  const double tflops = gemm_ms > 0 ? 2.0 * M * N * K * passes / (gemm_ms * 1e-3) / 1e12 : 0.0;
  printf("{\"check\":\"gemm\",%s\"ok\":%s,\"m\":%d,\"n\":%d,\"k\":%d,\"passes\":%d,\"mismatch_count\":%u,\"mismatches\":[%s],"
         "\"tflops\":%.3f}\n",
         fmt == MXFP8 ? "\"dtype\":\"mxfp8\"," : fmt == MXFP4 ? "\"dtype\":\"mxfp4\"," : fmt == FP64 ? "\"dtype\":\"fp64\"," : fmt == INT8 ? "\"dtype\":\"int8\"," : "",
         ok ? "true" : "false", M, N, K,
         passes, host.count, recs.c_str(), tflops);
  return ok ? 0 : 1;
}

static int run_hbm(double mib, int passes, uint32_t seed, bool flip, unsigned long long flip_word, uint32_t flip_mask,
                   int device) {
  if (passes < 1) return usage("hbm: --passes must be at least 1");
  CHECK(hipSetDevice(device));
  size_t free_b = 0, total_b = 0;
  CHECK(hipMemGetInfo(&free_b, &total_b));
  size_t bytes = mib > 0 ? static_cast<size_t>(mib * 1048576.0) : std::min(static_cast<size_t>(32) << 30, free_b / 2);
  bytes &= ~static_cast<size_t>(15);
  if (bytes < 16) return usage("hbm: --mib must give at least 16 bytes");
  if (flip && flip_word >= bytes / 4) return usage("hbm: --flip word outside the allocation");
  if (bytes > free_b) {  // never ask for more than is free: the check must not OOM another tenant
    fprintf(stderr, "hbm: %zu bytes asked, %zu free\n", bytes, free_b);
    printf("{\"check\":\"hbm\",\"ok\":false,\"error\":\"%zu bytes asked, %zu free\"}\n", bytes, free_b);
    return 3;
  }
  const int grid = grid_for(device);
  u32x4* p = nullptr;
  HbmResult* res = nullptr;
  CHECK(hipMalloc(&p, bytes));
  CHECK(hipMalloc(&res, sizeof(HbmResult)));
  CHECK(hipMemset(res, 0, sizeof(HbmResult)));
  hipEvent_t ev0, ev1;
  CHECK(hipEventCreate(&ev0));
  CHECK(hipEventCreate(&ev1));
  double ms_total = 0.0, moved = 0.0;
  // sweep `pass` checks pass-1 and writes pass; sweep `passes` only checks the last one
  for (int pass = 0; pass <= passes; ++pass) {
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(hbm_sweep_kernel, dim3(grid), dim3(256), 0, 0, p, bytes / 16, seed, pass - 1,
                       pass < passes ? pass : -1, res);
    CHECK(hipEventRecord(ev1));
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    ms_total += ms;
    moved += static_cast<double>(bytes) * ((pass > 0) + (pass < passes));
    if (pass == 0 && flip) {  // detector self-test: one word changed behind the kernel's back
      uint32_t word = 0;
      uint32_t* at = reinterpret_cast<uint32_t*>(p) + flip_word;
      CHECK(hipMemcpy(&word, at, 4, hipMemcpyDeviceToHost));
      word ^= flip_mask;
      CHECK(hipMemcpy(at, &word, 4, hipMemcpyHostToDevice));
    }
  }
  HbmResult host;
  CHECK(hipMemcpy(&host, res, sizeof(HbmResult), hipMemcpyDeviceToHost));
  CHECK(hipFree(p));
  const bool ok = host.count == 0;
  std::string recs;
  for (unsigned int r = 0; r < std::min(host.nrec, static_cast<unsigned int>(MAX_RECORDS)); ++r) {
    const HbmRecord& h = host.rec[r];
    char buf[160];
    snprintf(buf, sizeof buf, "{\"offset\":%llu,\"expected\":%u,\"got\":%u,\"xor\":%u}", h.offset, h.expected, h.got,
             h.expected ^ h.got);
    recs += (r ? "," : "") + std::string(buf);
  }
  printf("{\"check\":\"hbm\",\"ok\":%s,\"bytes\":%zu,\"passes\":%d,\"mismatch_count\":%llu,\"mismatches\":[%s],\"gbps\":%.1f}\n",
         ok ? "true" : "false", bytes, passes, host.count, recs.c_str(), ms_total > 0 ? moved / (ms_total * 1e-3) / 1e9 : 0.0);
  return ok ? 0 : 1;
}

struct CuPlace {  // HW_ID and XCC_ID decoded (the layout is in the kernel's comment)
  int xcc, se, sh, cu, simd;
  int cu_key() const { return ((xcc * 4 + se) * 2 + sh) * 16 + cu; }
};

static CuPlace cu_place(const CuWave& w) {
  return {static_cast<int>(w.xcc_id & 15u), static_cast<int>((w.hw_id >> 13) & 3u), static_cast<int>((w.hw_id >> 12) & 1u),
          static_cast<int>((w.hw_id >> 8) & 15u), static_cast<int>((w.hw_id >> 4) & 3u)};
}

static int run_cu(CuArgs a, int rounds, int device) {
  if (a.K < 16 || a.K % 16 || a.K > CU_K_CAP) return usage("cu: --k must be a multiple of 16, from 16 to 304");
  if (a.reps < 1 || a.passes < 1 || rounds < 1 || rounds > 64)
    return usage("cu: --reps and --passes must be at least 1, --rounds from 1 to 64");
  if (a.flip_wg >= 0 && a.flip_word >= CU_LDS_WORDS) return usage("cu: --flip word outside the 40960 words of LDS");
  if (a.poison_wg >= 0 && (a.poison_wave >= CU_WAVES || a.poison_i >= 32 || a.poison_j >= 32))
    return usage("cu: --poison wants a wave below 16 and I,J inside the 32x32 block");
  CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, device));
  const int cus = prop.multiProcessorCount;
  if (a.flip_wg >= cus || a.poison_wg >= cus) return usage("cu: --flip / --poison workgroup past the device's CUs");
  CuResult* res = nullptr;
  const size_t res_bytes = static_cast<size_t>(cus) * sizeof(CuResult);
  CHECK(hipMalloc(&res, res_bytes));
  hipEvent_t ev0, ev1;
  CHECK(hipEventCreate(&ev0));
  CHECK(hipEventCreate(&ev1));

  std::vector<CuResult> host(cus);
  std::vector<bool> seen_cu(8192, false), seen_simd(4 * 8192, false);
  int covered = 0, simds = 0, done = 0, nbad = 0;
  double ms_total = 0.0;
  std::string bad, placement;
  const CuArgs first = a;
  for (int round = 0; round < rounds && (covered < cus || simds < 4 * cus); ++round) {
    a = first;
    a.seed = first.seed + static_cast<uint32_t>(round);
    if (round > 0) a.flip_wg = a.poison_wg = -1;  // the self-tests alter round 0 only
    CHECK(hipMemset(res, 0, res_bytes));
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(cu_check_kernel, dim3(cus), dim3(CU_THREADS), 0, 0, res, a);
    CHECK(hipEventRecord(ev1));
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(host.data(), res, res_bytes, hipMemcpyDeviceToHost));
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    ms_total += ms;
    ++done;
    int spread[5] = {0, 0, 0, 0, 0}, strays = 0;  // workgroups by the number of SIMDs their waves ran on
    int fewest = CU_WAVES, most = 0;              // waves of one workgroup on one SIMD
    for (int wg = 0; wg < cus; ++wg) {
      const CuWave* w = host[wg].wave;
      const CuPlace at = cu_place(w[0]);
      unsigned long long lds_count = 0, mfma_count = 0;
      int lds_w = -1, mfma_w = -1, mask = 0, on[4] = {0, 0, 0, 0};
      for (int x = 0; x < CU_WAVES; ++x) {
        const CuPlace p = cu_place(w[x]);
        strays += p.cu_key() != at.cu_key();  // a workgroup's waves share a CU: anything else is a wrong decode
        mask |= 1 << p.simd;
        ++on[p.simd];
        if (!seen_cu[p.cu_key()]) seen_cu[p.cu_key()] = true, ++covered;
        if (!seen_simd[p.cu_key() * 4 + p.simd]) seen_simd[p.cu_key() * 4 + p.simd] = true, ++simds;
        lds_count += w[x].lds_count;
        mfma_count += w[x].mfma_count;
        if (w[x].lds_count && (lds_w < 0 || w[x].lds_offset < w[lds_w].lds_offset)) lds_w = x;
        if (w[x].mfma_count && mfma_w < 0) mfma_w = x;
      }
      ++spread[__builtin_popcount(mask)];
      fewest = std::min(fewest, *std::min_element(on, on + 4));
      most = std::max(most, *std::max_element(on, on + 4));
      if (lds_w < 0 && mfma_w < 0) continue;
      if (nbad++ >= MAX_RECORDS) continue;
      char buf[400];
      int n = snprintf(buf, sizeof buf, "%s{\"xcc\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d,\"wg\":%d,\"round\":%d", nbad > 1 ? "," : "",
                       at.xcc, at.se, at.sh, at.cu, wg, round);
      if (lds_w >= 0)
        n += snprintf(buf + n, sizeof buf - n, ",\"lds\":{\"count\":%llu,\"offset\":%u,\"expected\":%u,\"got\":%u,\"xor\":%u}",
                      lds_count, w[lds_w].lds_offset, w[lds_w].lds_expected, w[lds_w].lds_got,
                      w[lds_w].lds_expected ^ w[lds_w].lds_got);
      if (mfma_w >= 0)
        n += snprintf(buf + n, sizeof buf - n, ",\"mfma\":{\"count\":%llu,\"simd\":%d,\"i\":%d,\"j\":%d,\"delta\":%d}", mfma_count,
                      cu_place(w[mfma_w]).simd, w[mfma_w].mfma_i, w[mfma_w].mfma_j, w[mfma_w].mfma_delta);
      bad += std::string(buf) + "}";
    }
    char buf[256];
    snprintf(buf, sizeof buf, "%s{\"round\":%d,\"ms\":%.3f,\"covered\":%d,\"simds\":%d,\"wgs_on_1_2_3_4_simds\":[%d,%d,%d,%d],"
             "\"waves_per_simd\":[%d,%d],\"strays\":%d}",
             round ? "," : "", round, ms, covered, simds, spread[1], spread[2], spread[3], spread[4], fewest, most, strays);
    placement += buf;
  }
  CHECK(hipFree(res));
  const bool reached = covered == cus && simds == 4 * cus;
  const bool ok = reached && nbad == 0;
  printf("{\"check\":\"cu\",\"ok\":%s,%s\"cus\":%d,\"covered\":%d,\"simds\":%d,\"rounds\":%d,\"k\":%d,\"reps\":%d,\"passes\":%d,"
         "\"lds_bytes\":%d,\"bad_count\":%d,\"bad\":[%s],\"placement\":[%s],\"ms\":%.3f}\n",
         ok ? "true" : "false", reached ? "" : "\"error\":\"coverage\",", cus, covered, simds, done, first.K, first.reps,
         first.passes, CU_LDS_BYTES, nbad, bad.c_str(), placement.c_str(), ms_total);
  return ok ? 0 : 1;
}

// rows x D raw little-endian bf16 of Q: every element an integer, every row's magnitudes summing to at most 3
static bool read_q(const std::string& path, size_t rows, int D, std::vector<uint16_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out->resize(rows * D);
  const size_t got = fread(out->data(), 2, out->size(), f);
  const bool exact = got == out->size() && fgetc(f) == EOF;
  fclose(f);
  if (!exact) return false;
  for (size_t r = 0; r < rows; ++r) {
    int sum = 0;
    for (int c = 0; c < D; ++c) {
      int v;
      if (!bf16_whole((*out)[r * D + c], &v)) return false;
      sum += v < 0 ? -v : v;
    }
    if (sum > 3) return false;
  }
  return true;
}

static bool write_file(const std::string& path, const void* dev, size_t bytes) {
  std::vector<unsigned char> h(bytes);
  CHECK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && fwrite(h.data(), 1, bytes, f) == bytes;
  if (f) fclose(f);
  return ok;
}

static int run_attn(int H, int S, int D, bool causal, uint32_t seed, const std::string& q_file, const std::string& k_file,
                    const std::string& v_file, const std::string& o_out, const std::string& ml_out, int poison_h,
                    int poison_i, int poison_c, int device, double seconds) {
  // the caps of the exactness argument in the header: 2 S 2^12 <= 2^24
  if (S <= 0 || S % AT_KEYS || S > AT_S_CAP || (D != 64 && D != 128) || H < 1 || H > 65535)
    return usage("attn: S must be a multiple of 64 and at most 2048, d 64 or 128, H from 1 to 65535 (attn)");
  if (q_file.empty() != k_file.empty() || q_file.empty() != v_file.empty()) return usage("attn: --q, --k and --v go together (attn)");
  if (poison_h >= H || poison_i >= S || poison_c >= D) return usage("attn: --poison outside O' (attn)");
  const size_t rows = static_cast<size_t>(H) * S, elems = rows * D;
  std::vector<uint16_t> hq, hk, hv;
  if (!q_file.empty() && !(read_q(q_file, rows, D, &hq) && read_operand(k_file, elems, &hk) && read_operand(v_file, elems, &hv)))
    return usage("attn: --q/--k/--v must hold exactly H*S*d bf16 each: K and V integers in [-2, 2], every row of Q integers "
                 "whose magnitudes sum to at most 3 (attn)");

  CHECK(hipSetDevice(device));
  const int grid = grid_for(device);
  uint16_t *Q = nullptr, *K = nullptr, *V = nullptr;
  float *O = nullptr, *ML = nullptr;
  int *ofix = nullptr, *mlfix = nullptr;
  AttnResult* res = nullptr;
  CHECK(hipMalloc(&Q, elems * 2));
  CHECK(hipMalloc(&K, elems * 2));
  CHECK(hipMalloc(&V, elems * 2));
  CHECK(hipMalloc(&O, elems * 4));
  CHECK(hipMalloc(&ML, rows * 2 * 4));
  CHECK(hipMalloc(&ofix, elems * 4));
  CHECK(hipMalloc(&mlfix, rows * 2 * 4));
  CHECK(hipMalloc(&res, sizeof(AttnResult)));
  if (!q_file.empty()) {
    CHECK(hipMemcpy(Q, hq.data(), elems * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(K, hk.data(), elems * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(V, hv.data(), elems * 2, hipMemcpyHostToDevice));
  } else {
    hipLaunchKernelGGL(generate_q_kernel, dim3(grid), dim3(256), 0, 0, Q, rows, D, mix32(3 * seed));
    hipLaunchKernelGGL(generate_kernel, dim3(grid), dim3(256), 0, 0, K, static_cast<int>(rows), D, mix32(3 * seed + 1));
    hipLaunchKernelGGL(generate_kernel, dim3(grid), dim3(256), 0, 0, V, static_cast<int>(rows), D, mix32(3 * seed + 2));
  }
  // the inputs are the same in every pass, so the expectation is computed once
  hipLaunchKernelGGL(expect_attn_kernel, dim3(S, H), dim3(256), 0, 0, Q, K, V, S, D, causal ? 1 : 0, ofix, mlfix);
  CHECK(hipGetLastError());
  hipEvent_t ev0, ev1;
  CHECK(hipEventCreate(&ev0));
  CHECK(hipEventCreate(&ev1));

  AttnResult host = {};
  int passes = 0;
  double attn_ms = 0.0;
  const dim3 blocks((S + AT_QROWS - 1) / AT_QROWS, H);
  const auto t0 = std::chrono::steady_clock::now();
  do {
    CHECK(hipMemset(res, 0, sizeof(AttnResult)));
    CHECK(hipEventRecord(ev0));
    if (D == 64 && !causal) hipLaunchKernelGGL((attn_kernel<64, false>), blocks, dim3(256), 0, 0, Q, K, V, S, O, ML, poison_h, poison_i, poison_c);
    else if (D == 64) hipLaunchKernelGGL((attn_kernel<64, true>), blocks, dim3(256), 0, 0, Q, K, V, S, O, ML, poison_h, poison_i, poison_c);
    else if (!causal) hipLaunchKernelGGL((attn_kernel<128, false>), blocks, dim3(256), 0, 0, Q, K, V, S, O, ML, poison_h, poison_i, poison_c);
    else hipLaunchKernelGGL((attn_kernel<128, true>), blocks, dim3(256), 0, 0, Q, K, V, S, O, ML, poison_h, poison_i, poison_c);
    CHECK(hipEventRecord(ev1));
    hipLaunchKernelGGL(verify_attn_kernel, dim3(grid), dim3(256), 0, 0, O, ofix, ML, mlfix, elems, rows * 2, S, D, res);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(&host, res, sizeof(AttnResult), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    attn_ms += ms;
    ++passes;
  } while (host.count == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);

  if (!o_out.empty() && !write_file(o_out, O, elems * 4)) return usage("attn: cannot write --o-out (attn)");
  if (!ml_out.empty() && !write_file(ml_out, ML, rows * 2 * 4)) return usage("attn: cannot write --ml-out (attn)");
  const bool ok = host.count == 0;
  // wrong O' elements first, then l and m, each list in index order (the slots were taken in any order)
  const auto before = [](const AttnRecord& a, const AttnRecord& b) {
    return a.head != b.head ? a.head < b.head : a.i != b.i ? a.i < b.i : a.c != b.c ? a.c < b.c : a.kind < b.kind;
  };
  const unsigned int no = std::min(host.no, static_cast<unsigned int>(MAX_RECORDS));
  const unsigned int nml = std::min(host.nml, static_cast<unsigned int>(MAX_RECORDS) - no);
  std::sort(host.o, host.o + no, before);
  std::sort(host.ml, host.ml + std::min(host.nml, static_cast<unsigned int>(MAX_RECORDS)), before);
  std::string recs;
  for (unsigned int r = 0; r < no + nml; ++r) {
    const AttnRecord& a = r < no ? host.o[r] : host.ml[r - no];
    char buf[160];
    snprintf(buf, sizeof buf, "{\"kind\":\"%s\",\"head\":%d,\"i\":%d,\"c\":%d,\"delta\":%d}", a.kind == 0 ? "o" : a.kind == 1 ? "l" : "m",
             a.head, a.i, a.c, a.delta);
    recs += (r ? "," : "") + std::string(buf);
  }
  const double flops = 4.0 * S * S * D * H * (causal ? 0.5 : 1.0);
  printf("{\"check\":\"attn\",\"ok\":%s,\"heads\":%d,\"seq\":%d,\"d\":%d,\"causal\":%s,\"passes\":%d,\"mismatch_count\":%u,"
         "\"mismatches\":[%s],\"tflops\":%.3f}\n",
         ok ? "true" : "false", H, S, D, causal ? "true" : "false", passes, host.count, recs.c_str(),
         attn_ms > 0 ? flops * passes / (attn_ms * 1e-3) / 1e12 : 0.0);
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage("a subcommand is needed");
  const std::string mode = argv[1];
  if (mode != "gemm" && mode != "hbm" && mode != "cu" && mode != "attn") return usage("unknown subcommand");
  g_check = mode == "gemm" ? "gemm" : mode == "hbm" ? "hbm" : mode == "cu" ? "cu" : "attn";
  const bool cu = mode == "cu", attn = mode == "attn";
  int heads = 64, seq = AT_S_CAP, head_dim = 128, poison_h = -1, poison_c = -1;  // attn only
  bool causal = false;
  std::string q_file, k_file, v_file, o_out, ml_out;
  int fmt = BF16, M = 8192, N = 8192, K = 0, device = 0, passes = cu ? 4 : 2, poison_i = -1, poison_j = -1;
  int reps = 16, rounds = 8, flip_wg = -1, poison_wg = -1, poison_wave = 0;  // cu only
  double seconds = 2.0, mib = 0.0;
  uint32_t seed = 1, flip_mask = 0;
  unsigned long long flip_word = 0;
  bool flip = false;
  std::string a_file, b_file, sa_file, sb_file, c_out;
  for (int i = 2; i < argc; i += 2) {
    const std::string k = argv[i];
    if (attn && k == "--causal") {  // the one option without a value
      causal = true;
      --i;
      continue;
    }
    if (i + 1 >= argc) return usage(("option " + k + " needs a value").c_str());
    const char* v = argv[i + 1];
    char* end = nullptr;
    const bool gemm = mode == "gemm";
    if (attn) {
      if (k == "--device") device = atoi(v);
      else if (k == "--seed") seed = static_cast<uint32_t>(strtoul(v, nullptr, 0));
      else if (k == "--seconds") seconds = atof(v);
      else if (k == "--heads") heads = atoi(v);
      else if (k == "--seq") seq = atoi(v);
      else if (k == "--d") head_dim = atoi(v);
      else if (k == "--q") q_file = v;
      else if (k == "--k") k_file = v;
      else if (k == "--v") v_file = v;
      else if (k == "--o-out") o_out = v;
      else if (k == "--ml-out") ml_out = v;
      else if (k == "--poison") {
        poison_h = static_cast<int>(strtol(v, &end, 10));
        if (*end != ',' || poison_h < 0) return usage("--poison wants H,I,C (attn)");
        poison_i = static_cast<int>(strtol(end + 1, &end, 10));
        if (*end != ',' || poison_i < 0) return usage("--poison wants H,I,C (attn)");
        poison_c = static_cast<int>(strtol(end + 1, &end, 10));
        if (*end != '\0' || poison_c < 0) return usage("--poison wants H,I,C (attn)");
      } else return usage(("unknown option " + k + " (attn)").c_str());
      continue;
    }
    if (k == "--device") device = atoi(v);
    else if (k == "--seed") seed = static_cast<uint32_t>(strtoul(v, nullptr, 0));
    else if (cu && k == "--reps") reps = atoi(v);
    else if (cu && k == "--rounds") rounds = atoi(v);
    else if (cu && k == "--flip") {
      flip_wg = static_cast<int>(strtol(v, &end, 0));
      if (*end != ':' || flip_wg < 0) return usage("--flip wants WG:WORD:MASK");
      flip_word = strtoull(end + 1, &end, 0);
      if (*end != ':') return usage("--flip wants WG:WORD:MASK");
      flip_mask = static_cast<uint32_t>(strtoul(end + 1, &end, 0));
      if (*end != '\0' || flip_mask == 0) return usage("--flip wants WG:WORD:MASK with a non-zero mask");
    } else if (cu && k == "--poison") {
      poison_wg = static_cast<int>(strtol(v, &end, 10));
      if (*end != ':' || poison_wg < 0) return usage("--poison wants WG:WAVE:I,J");
      poison_wave = static_cast<int>(strtol(end + 1, &end, 10));
      if (*end != ':' || poison_wave < 0) return usage("--poison wants WG:WAVE:I,J");
      poison_i = static_cast<int>(strtol(end + 1, &end, 10));
      if (*end != ',' || poison_i < 0) return usage("--poison wants WG:WAVE:I,J");
      poison_j = static_cast<int>(strtol(end + 1, &end, 10));
      if (*end != '\0' || poison_j < 0) return usage("--poison wants WG:WAVE:I,J");
    }
    else if (gemm && k == "--m") M = atoi(v);
    else if (gemm && k == "--n") N = atoi(v);
    else if ((gemm || cu) && k == "--k") K = atoi(v);
    else if (gemm && k == "--a") a_file = v;
    else if (gemm && k == "--b") b_file = v;
    else if (gemm && k == "--sa") sa_file = v;
    else if (gemm && k == "--sb") sb_file = v;
    else if (gemm && k == "--dtype") {
      const std::string d = v;
      if (d != "bf16" && d != "mxfp8" && d != "mxfp4" && d != "fp64" && d != "int8")
        return usage("--dtype wants bf16, mxfp8, mxfp4, fp64 or int8");
      fmt = d == "bf16" ? BF16 : d == "mxfp8" ? MXFP8 : d == "mxfp4" ? MXFP4 : d == "fp64" ? FP64 : INT8;
    }
    else if (gemm && k == "--c-out") c_out = v;
    else if (gemm && k == "--seconds") seconds = atof(v);
    else if (gemm && k == "--poison") {
      poison_i = static_cast<int>(strtol(v, &end, 10));
      if (*end != ',' || poison_i < 0) return usage("--poison wants I,J");
      poison_j = static_cast<int>(strtol(end + 1, &end, 10));
      if (*end != '\0' || poison_j < 0) return usage("--poison wants I,J");
    } else if (!gemm && !cu && k == "--mib") {
      mib = atof(v);
      if (!(mib > 0)) return usage("--mib must be positive");
    } else if (!gemm && k == "--passes") passes = atoi(v);
    else if (!gemm && !cu && k == "--flip") {
      flip_word = strtoull(v, &end, 0);
      if (*end != ':') return usage("--flip wants WORD:MASK");
      flip_mask = static_cast<uint32_t>(strtoul(end + 1, &end, 0));
      if (*end != '\0' || flip_mask == 0) return usage("--flip wants WORD:MASK with a non-zero mask");
      flip = true;
    } else return usage(("unknown option " + k).c_str());
  }
  if (device < 0) return usage("--device must not be negative");
  if (attn)
    return run_attn(heads, seq, head_dim, causal, seed, q_file, k_file, v_file, o_out, ml_out, poison_h, poison_i, poison_c,
                    device, seconds);
  if (cu) {
    flip_word = std::min(flip_word, static_cast<unsigned long long>(CU_LDS_WORDS));  // a word past the LDS is refused below
    const CuArgs a = {seed,      passes,    K == 0 ? CU_K_CAP : K, reps,    flip_wg, static_cast<int>(flip_word),
                      flip_mask, poison_wg, poison_wave,           poison_i, poison_j};  // the default K is the cap
    return run_cu(a, rounds, device);
  }
  if (K == 0) K = fmt == BF16 || fmt == FP64 ? 4096 : fmt == MXFP8 || fmt == INT8 ? 8192 : 2048;  // the default: for the mx types the format's cap
  if (mode == "gemm")
    return run_gemm(fmt, M, N, K, seed, a_file, b_file, sa_file, sb_file, c_out, poison_i, poison_j, device, seconds);
  return run_hbm(mib, passes, seed, flip, flip_word, flip_mask, device);
}
