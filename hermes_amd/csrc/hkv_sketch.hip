// hkv_sketch.hip -- the invertible sketch of hermeskv.h "Sketch-level delta repair": folding a list of key summaries
// into 3 S cells, and the decode of the difference of two sketches. No table is involved; the C entry points are
// here too, ordered by their stream alone (like hkv_part_rows_diff_async).
//
// Fold: one summary per thread, 16 B loaded, and 12 no-return 64-bit atomics (add on the count, xor on the other
// three words) on its three cells. They execute at the memory side; a repair's sketch is a few MB and its list
// about a million summaries, so the adds spread over many lines.
//
// Decode: one subtract kernel, HKV_SKETCH_MAX_PASSES pass kernels and one closing kernel, all enqueued at once.
// Pass p owns subtable p mod 3: one cell per thread, read with plain loads (nothing else writes that subtable
// during the pass: an element has one cell there, and it is the pure cell its own thread clears), the element taken
// out of the other two subtables with no-return atomics. The word `passes` of the result carries the index of the
// last pass that took anything, plus 1, raised by an atomic max from every block that took one; a pass kernel that
// reads passes + 3 <= p returns at once. A block of pass p that reads the word while another block of the same pass
// raises it to p + 1 decides the same (the pass runs either way), so no kernel waits for another block's write.
// The lists are compacted as k_table_need compacts: a ballot per wave, the waves' totals through LDS, one returning
// atomic per block, step and list.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/hermeskv.h"
#include "hkv_internal.h"

namespace hkv {
namespace {
constexpr uint64_t kMixG = 0x9E3779B97F4A7C15ull;
constexpr int kSketchBlock = 256;
// word indices of hkv_sketch_result
enum : int { kSkOnlyA = 0, kSkOnlyB = 1, kSkUndecoded = 2, kSkPasses = 3, kSkExhausted = 4 };
using U = unsigned long long;

__device__ __forceinline__ uint64_t mix64(uint64_t x)   // the splitmix64 finaliser (the census's)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ uint64_t check_of(uint64_t a, uint64_t b) { return mix64(mix64(a + kMixG) + b); }
// the element's cell within subtable j (0 <= result < S < 2^32)
__device__ __forceinline__ uint64_t slot_of(uint64_t c, uint32_t j, uint64_t S)
{
    return ((mix64(c + (uint64_t)(j + 1) * kMixG) >> 32) * S) >> 32;
}
// cell += sign * element (sign 1 or 2^64 - 1), results unused: no-return atomics
__device__ __forceinline__ void cell_apply(U *cell, uint64_t sign, uint64_t a, uint64_t b, uint64_t c)
{
    atomicAdd(cell + 0, (U)sign);
    atomicXor(cell + 1, (U)a);
    atomicXor(cell + 2, (U)b);
    atomicXor(cell + 3, (U)c);
}

__global__ __launch_bounds__(kSketchBlock) void k_sketch_fold(const uint4 *__restrict__ summaries, uint64_t n,
                                                              U *__restrict__ cells, uint64_t S)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kSketchBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSketchBlock) {
        const uint4 sm = summaries[i];
        const uint64_t a = (uint64_t)sm.x | ((uint64_t)sm.y << 32), b = (uint64_t)sm.z | ((uint64_t)sm.w << 32);
        const uint64_t c = check_of(a, b);
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) cell_apply(cells + 4 * (j * S + slot_of(c, j, S)), 1ull, a, b, c);
    }
}

// a -= b over all 3 S cells, one cell (two 16-B halves) per thread
__global__ __launch_bounds__(kSketchBlock) void k_sketch_subtract(uint4 *__restrict__ a, const uint4 *__restrict__ b,
                                                                  uint64_t cells)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kSketchBlock + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * kSketchBlock) {
        uint4 x0 = a[2 * i], x1 = a[2 * i + 1];
        const uint4 y0 = b[2 * i], y1 = b[2 * i + 1];
        const uint64_t cnt = ((uint64_t)x0.x | ((uint64_t)x0.y << 32)) - ((uint64_t)y0.x | ((uint64_t)y0.y << 32));
        x0 = make_uint4((uint32_t)cnt, (uint32_t)(cnt >> 32), x0.z ^ y0.z, x0.w ^ y0.w);
        x1 = make_uint4(x1.x ^ y1.x, x1.y ^ y1.y, x1.z ^ y1.z, x1.w ^ y1.w);
        a[2 * i] = x0, a[2 * i + 1] = x1;
    }
}

__global__ __launch_bounds__(kSketchBlock) void k_sketch_pass(uint4 *__restrict__ cells, uint64_t S, uint32_t p,
                                                              uint4 *__restrict__ only_a, uint64_t cap_a,
                                                              uint4 *__restrict__ only_b, uint64_t cap_b, U *result)
{
    // (block-uniform, and the same in every block of the pass: see the head of the file)
    if (p >= 3 && __hip_atomic_load(&result[kSkPasses], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 3 <= p) return;
    const uint32_t j = p % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ U s_wtot[2][kSketchBlock / 64], s_base[2];
    U *const words = reinterpret_cast<U *>(cells);
    bool any = false;   // (thread 0's: the block took an element)
    for (uint64_t i0 = (uint64_t)blockIdx.x * kSketchBlock; i0 < S; i0 += (uint64_t)gridDim.x * kSketchBlock) {   // (block-uniform)
        const uint64_t i = i0 + threadIdx.x;
        uint64_t cnt = 0, a = 0, b = 0, c = 0;
        bool pure = false;
        if (i < S) {
            const uint4 x0 = cells[2 * (j * S + i)], x1 = cells[2 * (j * S + i) + 1];
            cnt = (uint64_t)x0.x | ((uint64_t)x0.y << 32), a = (uint64_t)x0.z | ((uint64_t)x0.w << 32);
            b = (uint64_t)x1.x | ((uint64_t)x1.y << 32), c = (uint64_t)x1.z | ((uint64_t)x1.w << 32);
            pure = (cnt == 1ull || cnt == ~0ull) && check_of(a, b) == c && slot_of(c, j, S) == i;
        }
        if (pure) {
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
            cells[2 * (j * S + i)] = z, cells[2 * (j * S + i) + 1] = z;
            const uint64_t sign = 0ull - cnt;   // the cells lose the pure cell's count
            cell_apply(words + 4 * (j1 * S + slot_of(c, j1, S)), sign, a, b, c);
            cell_apply(words + 4 * (j2 * S + slot_of(c, j2, S)), sign, a, b, c);
        }
        const bool to_a = pure && cnt == 1ull, to_b = pure && cnt != 1ull;
        const U bm_a = __ballot(to_a), bm_b = __ballot(to_b);
        if (lane == 0) s_wtot[0][wave] = (U)__popcll(bm_a), s_wtot[1][wave] = (U)__popcll(bm_b);
        __syncthreads();
        const U below = (1ull << lane) - 1;
        uint64_t before_a = (uint64_t)__popcll(bm_a & below), before_b = (uint64_t)__popcll(bm_b & below);
        uint64_t total_a = 0, total_b = 0;
#pragma unroll
        for (int w = 0; w < kSketchBlock / 64; ++w) {
            const U ta = s_wtot[0][w], tb = s_wtot[1][w];
            if (w < wave) before_a += ta, before_b += tb;
            total_a += ta, total_b += tb;
        }
        if (threadIdx.x == 0) {
            s_base[0] = total_a ? atomicAdd(&result[kSkOnlyA], (U)total_a) : 0ull;
            s_base[1] = total_b ? atomicAdd(&result[kSkOnlyB], (U)total_b) : 0ull;
            any |= (total_a | total_b) != 0;
        }
        __syncthreads();
        const uint4 el = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
        if (to_a && s_base[0] + before_a < cap_a) only_a[s_base[0] + before_a] = el;
        if (to_b && s_base[1] + before_b < cap_b) only_b[s_base[1] + before_b] = el;
    }
    if (threadIdx.x == 0 && any) atomicMax(&result[kSkPasses], (U)p + 1);
}

// the non-zero cells left, and whether the passes ran out
__global__ __launch_bounds__(kSketchBlock) void k_sketch_close(const uint4 *__restrict__ cells, uint64_t n_cells, U *result)
{
    __shared__ U s_wtot[kSketchBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSketchBlock + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * kSketchBlock) {
        const uint4 x0 = cells[2 * i], x1 = cells[2 * i + 1];
        mine += ((x0.x | x0.y | x0.z | x0.w | x1.x | x1.y | x1.z | x1.w) != 0u);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d);
    if (lane == 0) s_wtot[wave] = (U)mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        U t = 0;
#pragma unroll
        for (int w = 0; w < kSketchBlock / 64; ++w) t += s_wtot[w];
        if (t) atomicAdd(&result[kSkUndecoded], t);
        if (blockIdx.x == 0 && result[kSkPasses] + 3 > (U)HKV_SKETCH_MAX_PASSES) result[kSkExhausted] = 1ull;
    }
}

dim3 sketch_grid(uint64_t items, int device)
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    const uint64_t steps = (items + kSketchBlock - 1) / kSketchBlock, most = (uint64_t)cus * 8;
    return dim3((unsigned)(steps < most ? (steps ? steps : 1) : most));
}
}  // namespace

int launch_sketch_fold(const uint8_t *summaries, uint64_t n, void *cells, uint64_t S, int accumulate, int device,
                       hipStream_t s)
{
    if (!accumulate && hipMemsetAsync(cells, 0, 3 * S * sizeof(hkv_sketch_cell), s) != hipSuccess) return -2;
    if (!n) return 0;
    hipLaunchKernelGGL(k_sketch_fold, sketch_grid(n, device), dim3(kSketchBlock), 0, s,
                       reinterpret_cast<const uint4 *>(summaries), n, static_cast<U *>(cells), S);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_sketch_decode(void *a, const void *b, uint64_t S, uint8_t *only_a, uint64_t cap_a, uint8_t *only_b,
                         uint64_t cap_b, unsigned long long *result, int device, hipStream_t s)
{
    if (hipMemsetAsync(result, 0, sizeof(hkv_sketch_result), s) != hipSuccess) return -2;
    hipLaunchKernelGGL(k_sketch_subtract, sketch_grid(3 * S, device), dim3(kSketchBlock), 0, s, static_cast<uint4 *>(a),
                       static_cast<const uint4 *>(b), 3 * S);
    const dim3 grid = sketch_grid(S, device);
    for (uint32_t p = 0; p < (uint32_t)HKV_SKETCH_MAX_PASSES; ++p)
        hipLaunchKernelGGL(k_sketch_pass, grid, dim3(kSketchBlock), 0, s, static_cast<uint4 *>(a), S, p,
                           reinterpret_cast<uint4 *>(only_a), cap_a, reinterpret_cast<uint4 *>(only_b), cap_b, result);
    hipLaunchKernelGGL(k_sketch_close, sketch_grid(3 * S, device), dim3(kSketchBlock), 0, s,
                       static_cast<const uint4 *>(a), 3 * S, result);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace hkv

using namespace hkv;

static_assert(sizeof(hkv_sketch_cell) == 32 && sizeof(hkv_sketch_result) == 64, "the kernels' word indices");
uint32_t hkv_sketch_cell_bytes(void) { return (uint32_t)sizeof(hkv_sketch_cell); }
uint32_t hkv_sketch_result_bytes(void) { return (uint32_t)sizeof(hkv_sketch_result); }

static int sketch_fail(int code, const char *what, const char *msg)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, msg);
    return api_fail(code, buf);
}
static int sub_cells_ok(uint64_t S, const char *what)
{
    return S == 0 || S >= (1ull << 32) ? sketch_fail(-1, what, "sub_cells must be in [1, 2^32)") : 0;
}

int hkv_summaries_sketch_async(const void *d_summaries, uint64_t n, hkv_sketch_cell *d_cells, uint64_t sub_cells,
                               int accumulate, void *stream)
{
    const char *what = "sketch";
    if (!d_cells) return sketch_fail(-1, what, "null cells");
    if (n && !d_summaries) return sketch_fail(-1, what, "a count without its buffer");
    if (((uintptr_t)d_summaries | (uintptr_t)d_cells) & 15)
        return sketch_fail(-1, what, "the summaries and the cells must be 16-byte aligned");
    if (int rc = sub_cells_ok(sub_cells, what)) return rc;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return sketch_fail(-5, what, "hipGetDevice failed");
    if (int rc = launch_sketch_fold(static_cast<const uint8_t *>(d_summaries), n, d_cells, sub_cells, accumulate, device,
                                    (hipStream_t)stream))
        return sketch_fail(-3, what, rc == -2 ? "zeroing the cells failed" : hipGetErrorString(hipGetLastError()));
    return 0;
}

int hkv_sketch_decode_async(hkv_sketch_cell *d_a, const hkv_sketch_cell *d_b, uint64_t sub_cells, void *d_only_a,
                            uint64_t cap_a, void *d_only_b, uint64_t cap_b, hkv_sketch_result *d_result, void *stream)
{
    const char *what = "sketch_decode";
    if (!d_a || !d_b || !d_result) return sketch_fail(-1, what, "null cells or result");
    if ((cap_a && !d_only_a) || (cap_b && !d_only_b)) return sketch_fail(-1, what, "a cap without its buffer");
    if (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_only_a | (uintptr_t)d_only_b | (uintptr_t)d_result) & 15)
        return sketch_fail(-1, what, "the cells, the lists and d_result must be 16-byte aligned");
    if (int rc = sub_cells_ok(sub_cells, what)) return rc;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return sketch_fail(-5, what, "hipGetDevice failed");
    if (int rc = launch_sketch_decode(d_a, d_b, sub_cells, static_cast<uint8_t *>(d_only_a), cap_a,
                                      static_cast<uint8_t *>(d_only_b), cap_b,
                                      reinterpret_cast<unsigned long long *>(d_result), device, (hipStream_t)stream))
        return sketch_fail(-3, what, rc == -2 ? "zeroing d_result failed" : hipGetErrorString(hipGetLastError()));
    return 0;
}
