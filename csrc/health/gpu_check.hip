// gpu_check — an active device check with exact answers: "is this GPU bad, or was it the job?"
//
//   gpu_check gemm --m M --n N --k K [--seed S] [--a FILE --b FILE] [--c-out FILE]
//                  [--poison I,J] [--device D] [--seconds T]
//        bf16 x bf16 -> fp32 GEMM on the matrix units (v_mfma_f32_32x32x16_bf16), checked on
//        the device by Huang-Abraham checksums.  Every element of A (M x K, row-major) and
//        B (N x K, K-contiguous) is an integer in [-2, 2], so every product, partial sum and
//        checksum is an integer of magnitude <= 4*K*128 <= 2^24 and fp32 holds it exactly in
//        any summation order: a healthy device agrees bit for bit with integer arithmetic and
//        the comparison is ==, no tolerance.  The expected checksums come from integer kernels
//        that share nothing with the matrix path.
//   gpu_check hbm --mib SIZE [--passes P] [--seed S] [--flip WORD:MASK] [--device D]
//        moving inversions over one allocation: pass 0 writes an address hash, each later pass
//        loads, compares with what the pass before wrote and stores the next pattern (odd
//        passes store the bitwise complement, so every cell is held in both states); a last
//        read-only sweep checks what the final pass wrote.
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

// ------------------------------------------------------------------------------------------
// The GEMM with checksum epilogue
// ------------------------------------------------------------------------------------------

constexpr int TILE = 128;                  // C tile edge per workgroup
constexpr int KSTEP = 64;                  // K advance per LDS stage
constexpr int ROW_BYTES = KSTEP * 2 + 16;  // 128 B of data + 16 B pad
constexpr int STAGE_BYTES = TILE * ROW_BYTES;

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

  // Epilogue, from registers.  Element (bm, bn, r) of this lane is
  //   row  row0 + wm*64 + bm*32 + 8*(r/4) + 4*half + r%4,   column  col0 + wn*64 + bn*32 + l32.
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

  float* red = reinterpret_cast<float*>(lds);  // [0,256): column partials by wm; [256,512): row partials by wn
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

constexpr int MAX_RECORDS = 16;

struct Suspect {  // one checksum that disagrees
  int stripe, index;
  float delta;
};
struct GemmRecord {
  int kind;  // 0 element, 1 row, 2 column
  int i, j, tile;
  float delta;
};
struct GemmResult {
  unsigned int count, ncol, nrow, nrec;
  Suspect col[MAX_RECORDS], row[MAX_RECORDS];
  GemmRecord rec[MAX_RECORDS];
};

__global__ __launch_bounds__(256) void verify_kernel(const float* __restrict__ colsum, const int* __restrict__ colexp,
                                                     size_t ncol, int N, const float* __restrict__ rowsum,
                                                     const int* __restrict__ rowexp, size_t nrow, int M, GemmResult* res) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t x = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; x < ncol + nrow; x += stride) {
    const bool is_col = x < ncol;
    const size_t y = is_col ? x : x - ncol;
    const float got = is_col ? colsum[y] : rowsum[y];
    const float want = static_cast<float>(is_col ? colexp[y] : rowexp[y]);
    if (got == want) continue;  // a NaN is a mismatch
    atomicAdd(&res->count, 1u);
    const unsigned int slot = atomicAdd(is_col ? &res->ncol : &res->nrow, 1u);
    if (slot < MAX_RECORDS) {
      const int width = is_col ? N : M;
      Suspect sus = {static_cast<int>(y / width), static_cast<int>(y % width), got - want};
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
// Host
// ------------------------------------------------------------------------------------------

static int grid_for(int dev) {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, dev));
  return prop.multiProcessorCount * 8;
}

static int usage(const char* why) {
  fprintf(stderr,
          "%s\nusage: gpu_check gemm --m M --n N --k K [--seed S] [--a FILE --b FILE] [--c-out FILE] [--poison I,J] "
          "[--device D] [--seconds T]\n       gpu_check hbm --mib SIZE [--passes P] [--seed S] [--flip WORD:MASK] "
          "[--device D]\n",
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

static int run_gemm(int M, int N, int K, uint32_t seed, const std::string& a_file, const std::string& b_file,
                    const std::string& c_out, int poison_i, int poison_j, int device, double seconds) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 16 || K > 32768)
    return usage("gemm: M and N must be multiples of 32, K a multiple of 16 and at most 32768");
  if (a_file.empty() != b_file.empty()) return usage("gemm: --a and --b go together");
  if (poison_i >= M || poison_j >= N) return usage("gemm: --poison outside C");
  const size_t a_elems = static_cast<size_t>(M) * K, b_elems = static_cast<size_t>(N) * K;
  std::vector<uint16_t> ha, hb;
  if (!a_file.empty() && !(read_operand(a_file, a_elems, &ha) && read_operand(b_file, b_elems, &hb)))
    return usage("gemm: --a/--b must hold exactly M*K and N*K bf16 integers in [-2, 2]");

  CHECK(hipSetDevice(device));
  const int grid = grid_for(device);
  const int tiles_m = (M + TILE - 1) / TILE, tiles_n = (N + TILE - 1) / TILE;
  const size_t ncol = static_cast<size_t>(tiles_m) * N, nrow = static_cast<size_t>(tiles_n) * M;
  uint16_t *A = nullptr, *B = nullptr;
  float *colsum = nullptr, *rowsum = nullptr, *C = nullptr;
  int *ea = nullptr, *eb = nullptr, *colexp = nullptr, *rowexp = nullptr;
  GemmResult* res = nullptr;
  CHECK(hipMalloc(&A, a_elems * 2));
  CHECK(hipMalloc(&B, b_elems * 2));
  CHECK(hipMalloc(&colsum, ncol * 4));
  CHECK(hipMalloc(&rowsum, nrow * 4));
  CHECK(hipMalloc(&colexp, ncol * 4));
  CHECK(hipMalloc(&rowexp, nrow * 4));
  CHECK(hipMalloc(&ea, static_cast<size_t>(tiles_m) * K * 4));
  CHECK(hipMalloc(&eb, static_cast<size_t>(tiles_n) * K * 4));
  CHECK(hipMalloc(&res, sizeof(GemmResult)));
  if (!c_out.empty()) CHECK(hipMalloc(&C, static_cast<size_t>(M) * N * 4));
  if (!a_file.empty()) {
    CHECK(hipMemcpy(A, ha.data(), a_elems * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(B, hb.data(), b_elems * 2, hipMemcpyHostToDevice));
  }
  hipEvent_t ev0, ev1;
  CHECK(hipEventCreate(&ev0));
  CHECK(hipEventCreate(&ev1));

  GemmResult host = {};
  int passes = 0;
  double gemm_ms = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  do {
    if (a_file.empty()) {
      const uint32_t s = seed + static_cast<uint32_t>(passes);
      hipLaunchKernelGGL(generate_kernel, dim3(grid), dim3(256), 0, 0, A, M, K, mix32(2 * s));
      hipLaunchKernelGGL(generate_kernel, dim3(grid), dim3(256), 0, 0, B, N, K, mix32(2 * s + 1));
    }
    CHECK(hipMemset(res, 0, sizeof(GemmResult)));
    CHECK(hipEventRecord(ev0));
    hipLaunchKernelGGL(gemm_abft_kernel, dim3(tiles_n, tiles_m), dim3(256), 0, 0, A, B, M, N, K, colsum, rowsum, C,
                       poison_i, poison_j);
    CHECK(hipEventRecord(ev1));
    hipLaunchKernelGGL(stripe_sum_kernel, dim3((K + 255) / 256, tiles_m), dim3(256), 0, 0, A, M, K, ea);
    hipLaunchKernelGGL(stripe_sum_kernel, dim3((K + 255) / 256, tiles_n), dim3(256), 0, 0, B, N, K, eb);
    hipLaunchKernelGGL(expect_kernel, dim3(N, (tiles_m + 3) / 4), dim3(256), 0, 0, ea, tiles_m, B, N, K, colexp);
    hipLaunchKernelGGL(expect_kernel, dim3(M, (tiles_n + 3) / 4), dim3(256), 0, 0, eb, tiles_n, A, M, K, rowexp);
    hipLaunchKernelGGL(verify_kernel, dim3(grid), dim3(256), 0, 0, colsum, colexp, ncol, N, rowsum, rowexp, nrow, M, res);
    hipLaunchKernelGGL(locate_kernel, dim3(1), dim3(1), 0, 0, res, tiles_n);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(&host, res, sizeof(GemmResult), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    gemm_ms += ms;
    ++passes;
  } while (host.count == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);

  if (C != nullptr) {
    std::vector<float> hc(static_cast<size_t>(M) * N);
    CHECK(hipMemcpy(hc.data(), C, hc.size() * 4, hipMemcpyDeviceToHost));
    FILE* f = fopen(c_out.c_str(), "wb");
    if (!f || fwrite(hc.data(), 4, hc.size(), f) != hc.size()) return usage("gemm: cannot write --c-out");
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
  printf("{\"check\":\"gemm\",\"ok\":%s,\"m\":%d,\"n\":%d,\"k\":%d,\"passes\":%d,\"mismatch_count\":%u,\"mismatches\":[%s],"
         "\"tflops\":%.3f}\n",
         ok ? "true" : "false", M, N, K, passes, host.count, recs.c_str(), tflops);
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

int main(int argc, char** argv) {
  if (argc < 2) return usage("a subcommand is needed");
  const std::string mode = argv[1];
  if (mode != "gemm" && mode != "hbm") return usage("unknown subcommand");
  g_check = mode == "gemm" ? "gemm" : "hbm";
  int M = 8192, N = 8192, K = 4096, device = 0, passes = 2, poison_i = -1, poison_j = -1;
  double seconds = 2.0, mib = 0.0;
  uint32_t seed = 1, flip_mask = 0;
  unsigned long long flip_word = 0;
  bool flip = false;
  std::string a_file, b_file, c_out;
  for (int i = 2; i < argc; i += 2) {
    const std::string k = argv[i];
    if (i + 1 >= argc) return usage(("option " + k + " needs a value").c_str());
    const char* v = argv[i + 1];
    char* end = nullptr;
    const bool gemm = mode == "gemm";
    if (k == "--device") device = atoi(v);
    else if (k == "--seed") seed = static_cast<uint32_t>(strtoul(v, nullptr, 0));
    else if (gemm && k == "--m") M = atoi(v);
    else if (gemm && k == "--n") N = atoi(v);
    else if (gemm && k == "--k") K = atoi(v);
    else if (gemm && k == "--a") a_file = v;
    else if (gemm && k == "--b") b_file = v;
    else if (gemm && k == "--c-out") c_out = v;
    else if (gemm && k == "--seconds") seconds = atof(v);
    else if (gemm && k == "--poison") {
      poison_i = static_cast<int>(strtol(v, &end, 10));
      if (*end != ',' || poison_i < 0) return usage("--poison wants I,J");
      poison_j = static_cast<int>(strtol(end + 1, &end, 10));
      if (*end != '\0' || poison_j < 0) return usage("--poison wants I,J");
    } else if (!gemm && k == "--mib") {
      mib = atof(v);
      if (!(mib > 0)) return usage("--mib must be positive");
    } else if (!gemm && k == "--passes") passes = atoi(v);
    else if (!gemm && k == "--flip") {
      flip_word = strtoull(v, &end, 0);
      if (*end != ':') return usage("--flip wants WORD:MASK");
      flip_mask = static_cast<uint32_t>(strtoul(end + 1, &end, 0));
      if (*end != '\0' || flip_mask == 0) return usage("--flip wants WORD:MASK with a non-zero mask");
      flip = true;
    } else return usage(("unknown option " + k).c_str());
  }
  if (device < 0) return usage("--device must not be negative");
  if (mode == "gemm") return run_gemm(M, N, K, seed, a_file, b_file, c_out, poison_i, poison_j, device, seconds);
  return run_hbm(mib, passes, seed, flip, flip_word, flip_mask, device);
}
