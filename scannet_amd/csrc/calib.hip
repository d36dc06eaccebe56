// calib.hip -- PMC calibration helper: a plain 16 B-per-lane read-modify-write stream over a known byte
// count, the access pattern of k_integrate.  Used only to calibrate rocprofv3 FETCH_SIZE / WRITE_SIZE on
// gfx950 (MI355X_MICROARCH.md section HBM: FETCH_SIZE under-reports wide coalesced reads) -- see
// tools/pmc_calibrate.py and DESIGN.md section 5.
#include <hip/hip_runtime.h>

#include "common.h"
#include "fuser_internal.h"
#include "hip_util.h"

namespace {
__global__ __launch_bounds__(256) void k_calib_rmw(uint4* __restrict__ buf, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    uint4 v = buf[i];
    v.x += 1u; v.y ^= v.x; v.z += v.y; v.w ^= v.z;
    buf[i] = v;
  }
}
__global__ __launch_bounds__(256) void k_calib_read(const uint4* __restrict__ buf, size_t n16, uint32_t* sink) {
  uint32_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const uint4 v = buf[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x12345u) *sink = acc;
}
}  // namespace

// Runs `iters` launches of a read+write stream and `iters` of a read-only stream over `bytes` bytes.
SF_API int sf_calib_stream(int device, uint64_t bytes, int iters) {
  SF_HIP_CHECK(hipSetDevice(device));
  sf::DevBuf buf, sink;
  SF_HIP_CHECK(buf.alloc(bytes));
  SF_HIP_CHECK(sink.alloc(4));
  SF_HIP_CHECK(hipMemset(buf.p, 1, bytes));
  for (int i = 0; i < iters; i++) hipLaunchKernelGGL(k_calib_rmw, dim3(8192), dim3(256), 0, 0, buf.as<uint4>(), (size_t)(bytes / 16));
  for (int i = 0; i < iters; i++) hipLaunchKernelGGL(k_calib_read, dim3(8192), dim3(256), 0, 0, buf.as<uint4>(), (size_t)(bytes / 16), sink.as<uint32_t>());
  SF_HIP_CHECK(hipDeviceSynchronize());
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Device self-test of the hand-expanded divisions (fuser_internal.h) against the hardware's IEEE division:
//   recip: every one of the 2^23 mantissas at 9 exponents spanning 2^-20 .. 2^20 (camera-space depths in metres),
//   quot : every integer divisor 1..511 against 2^20 numerators each (counter-based bit patterns with exponents in the
//          TSDF range, plus exact multiples and their neighbours: the near-halfway quotients).
//   div  : k_alloc's general quotient div_rn(a, b, recip_rn(b)): 2^28 operand pairs -- counter-based bit patterns with both signs and
//          exponents 2^-24 .. 2^16 for the divisor (ray directions, the voxel size) and 2^-30 .. 2^12 for the dividend, plus for every pair
//          the dividends that sit within 3 ulp of an exact multiple and of a half-way multiple of the divisor (the hard cases of rounding).
// Returns the number of lanes whose result differs in any bit (expected: 0, 0 and 0).
// ---------------------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void k_selftest_recip(unsigned long long* bad) {
  const uint32_t mant = blockIdx.x * 256 + threadIdx.x;  // 2^23 threads
  const uint32_t expo[9] = {107, 117, 122, 126, 127, 128, 132, 137, 147};
  unsigned int n = 0;
  for (int e = 0; e < 9; e += 2) {
    const float b0 = __uint_as_float((expo[e] << 23) | mant), b1 = __uint_as_float((expo[(e + 1) % 9] << 23) | mant);
    const v2f r = recip_rn((v2f){b0, b1});
    n += __float_as_uint(r.x) != __float_as_uint(1.0f / b0);
    n += __float_as_uint(r.y) != __float_as_uint(1.0f / b1);
  }
  if (n) atomicAdd(bad, (unsigned long long)n);
}
__global__ __launch_bounds__(256) void k_selftest_quot(unsigned long long* bad) {
  const uint32_t m_int = blockIdx.y + 1;  // 1..511
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // 2^20 numerators per divisor
  const float m = (float)m_int, r = 1.0f / m;
  uint64_t x = ((uint64_t)m_int << 32 | i) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
  float n0, n1;
  {
    const uint32_t e = 100u + (uint32_t)(x >> 58);  // 2^-27 .. 2^36
    n0 = __uint_as_float(((uint32_t)x & 0x807FFFFFu) | (e << 23));
    const float qf = __uint_as_float(0x3F800000u | ((uint32_t)(x >> 24) & 0x7FFFFFu));  // quotient near 1..2
    n1 = __uint_as_float(__float_as_uint(qf * m) + ((uint32_t)(x >> 50) & 7u) - 3u);    // a multiple of m, +-3 ulp
  }
  const v2f q = quot_rn((v2f){n0, n1}, splat(m), splat(r));
  unsigned int n = (__float_as_uint(q.x) != __float_as_uint(n0 / m)) + (__float_as_uint(q.y) != __float_as_uint(n1 / m));
  if (n) atomicAdd(bad, (unsigned long long)n);
}
__global__ __launch_bounds__(256) void k_selftest_div(unsigned long long* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;   // 2^26 threads, 4 quotients each
  uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
  uint64_t y = (x ^ 0xD6E8FEB86659FD93ull) * 0x94D049BB133111EBull;
  y ^= y >> 31;
  const uint32_t eb = 103u + (uint32_t)(x >> 58) % 41u;          // divisor 2^-24 .. 2^16
  const uint32_t ea = 97u + (uint32_t)(y >> 58) % 43u;           // dividend 2^-30 .. 2^12
  const float b = __uint_as_float(((uint32_t)x & 0x807FFFFFu) | (eb << 23));
  const float a0 = __uint_as_float(((uint32_t)y & 0x807FFFFFu) | (ea << 23));
  const float qf = __uint_as_float(0x3F800000u | ((uint32_t)(y >> 24) & 0x7FFFFFu));                         // a quotient in [1, 2)
  const float a1 = __uint_as_float(__float_as_uint(qf * b) + ((uint32_t)(x >> 50) & 7u) - 3u);               // near an exact multiple of b
  const float qh = __uint_as_float(__float_as_uint(qf) & 0xFFFFFFFEu);                                       // even significand: qh + ulp/2 is half-way
  const float a2 = __uint_as_float(__float_as_uint(fmaf(qh, b, 0x1p-24f * b)) + ((uint32_t)(y >> 50) & 7u) - 3u);   // near a half-way quotient
  const float a3 = __uint_as_float(__float_as_uint(a0) ^ 0x00400000u);
  const float rb = recip_rn(b);
  unsigned int n = 0;
  n += __float_as_uint(div_rn(a0, b, rb)) != __float_as_uint(a0 / b);
  n += __float_as_uint(div_rn(a1, b, rb)) != __float_as_uint(a1 / b);
  n += __float_as_uint(div_rn(a2, b, rb)) != __float_as_uint(a2 / b);
  n += __float_as_uint(div_rn(a3, b, rb)) != __float_as_uint(a3 / b);
  n += __float_as_uint(rb) != __float_as_uint(1.0f / b);
  if (n) atomicAdd(bad, (unsigned long long)n);
}
// 1 / b by ONE Newton step from the v_rcp_f32 seed (recip_one_step, fuser_internal.h) for every one of the 2^32 bit patterns: 16 per thread.  Counted:
// normal b whose correctly rounded reciprocal is normal as well.  tools/check_division.c part (4) shows what the outcome hangs on: from a seed that
// is one of the two floats either side of 1 / b the step is exact for every mantissa but all-ones, and for that one from the round-up seed -- so
// whether the step suffices is a property of this part's v_rcp_f32, decided by running it.
__global__ __launch_bounds__(256) void k_selftest_recip_one_step(unsigned long long* bad, uint32_t* first, uint32_t capacity) {
  const uint32_t base = (blockIdx.x * 256u + threadIdx.x) << 4;   // 2^28 threads
  for (uint32_t k = 0; k < 16u; k++) {
    const uint32_t bits = base | k;
    const float b = __uint_as_float(bits);
    const uint32_t ref = __float_as_uint(1.0f / b);
    const uint32_t eb = (bits >> 23) & 0xFFu, er = (ref >> 23) & 0xFFu;
    if (eb == 0u || eb == 255u || er == 0u || er == 255u) continue;
    if (__float_as_uint(recip_one_step(b)) != ref) {
      const unsigned long long slot = atomicAdd(bad, 1ull);
      if (slot < (unsigned long long)capacity) first[slot] = bits;
    }
  }
}
// the per-weight records of k_integrate's LDS table, built by the function the kernel calls, copied out word for word
__global__ __launch_bounds__(256) void k_selftest_weight_records(uint4* out) {
  __shared__ uint4 s_rec[WREC];
  fill_weight_records(s_rec, (int)threadIdx.x, 256);
  __syncthreads();
  for (int i = threadIdx.x; i < WREC; i += 256) out[i] = s_rec[i];
}
}  // namespace

SF_API int sf_selftest_weight_records(int device, uint32_t* out) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(device));
  sf::DevBuf d;
  SF_HIP_CHECK(d.alloc(WREC * sizeof(uint4)));
  hipLaunchKernelGGL(k_selftest_weight_records, dim3(1), dim3(256), 0, nullptr, d.as<uint4>());
  SF_HIP_CHECK(hipGetLastError());
  SF_HIP_CHECK(hipMemcpy(out, d.p, WREC * sizeof(uint4), hipMemcpyDeviceToHost));
  return SF_OK;
}

SF_API int sf_selftest_recip_one_step(int device, uint64_t* mismatches, uint32_t* patterns_out, uint32_t capacity, int* shipped) {
  if (!mismatches || (capacity > 0 && !patterns_out)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(device));
  sf::DevBuf d, p;
  const size_t pbytes = 4 * (size_t)(capacity ? capacity : 1);
  SF_HIP_CHECK(d.alloc(8));
  SF_HIP_CHECK(p.alloc(pbytes));
  SF_HIP_CHECK(hipMemset(d.p, 0, 8));
  SF_HIP_CHECK(hipMemset(p.p, 0, pbytes));
  hipLaunchKernelGGL(k_selftest_recip_one_step, dim3(1u << 20), dim3(256), 0, nullptr, d.as<unsigned long long>(), p.as<uint32_t>(), capacity);
  SF_HIP_CHECK(hipGetLastError());
  unsigned long long h = 0;
  SF_HIP_CHECK(hipMemcpy(&h, d.p, 8, hipMemcpyDeviceToHost));
  if (capacity > 0) SF_HIP_CHECK(hipMemcpy(patterns_out, p.p, 4 * (size_t)capacity, hipMemcpyDeviceToHost));
  *mismatches = h;
  if (shipped) *shipped = RECIP_ONE_STEP ? 1 : 0;
  return SF_OK;
}

SF_API int sf_selftest_division(int device, uint64_t* recip_mismatches, uint64_t* quot_mismatches, uint64_t* div_mismatches) {
  if (!recip_mismatches || !quot_mismatches || !div_mismatches) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(device));
  sf::DevBuf buf;
  SF_HIP_CHECK(buf.alloc(24));
  SF_HIP_CHECK(hipMemset(buf.p, 0, 24));
  unsigned long long* d = buf.as<unsigned long long>();
  hipLaunchKernelGGL(k_selftest_recip, dim3((1u << 23) / 256), dim3(256), 0, nullptr, d);
  hipLaunchKernelGGL(k_selftest_quot, dim3((1u << 20) / 256, 511), dim3(256), 0, nullptr, d + 1);
  hipLaunchKernelGGL(k_selftest_div, dim3((1u << 26) / 256), dim3(256), 0, nullptr, d + 2);
  unsigned long long h[3] = {0, 0, 0};
  SF_HIP_CHECK(hipMemcpy(h, d, 24, hipMemcpyDeviceToHost));
  *recip_mismatches = h[0];
  *quot_mismatches = h[1];
  *div_mismatches = h[2];
  return SF_OK;
}
