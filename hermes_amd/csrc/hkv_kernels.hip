// hkv_kernels.hip -- CDNA4 (gfx950) kernels on the table itself: CityHash128 of key ids, populate, and (at the
// end) the inline residency's conversions, the table census and the replica repair's extract and install.
//
// Populate (spacetime.c:32-68 / mica.c:78-146): hash every id, sort the inserts by bucket (stable,
// so each bucket sees its inserts in insertion order), one owner lane per bucket replays the MICA
// slot rules, and the log entries are written in parallel. The batch path is in hkv_batch.hip and
// hkv_batch_small.hip.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "hkv_exec.h"
#include "hkv_internal.h"
#include "hkv_table_dev.h"

namespace hkv {

// ------------------------------------------------------------------ CityHash128, 4-byte keys
// city.c:85-400 restricted to the CityMurmur short-string path that mica_gen_keys uses.
__device__ __forceinline__ uint64_t ch_mix16(uint64_t u, uint64_t v)
{
    const uint64_t mul = 0x9ddfea08eb382d69ULL;
    uint64_t a = (u ^ v) * mul;
    a ^= a >> 47;
    uint64_t b = (v ^ a) * mul;
    b ^= b >> 47;
    return b * mul;
}

__device__ __forceinline__ void cityhash128_u32(uint32_t id, uint64_t &first, uint64_t &second)
{
    const uint64_t k0 = 0xc3a5c85c97cb3127ULL, k1 = 0xb492b66fbe98f273ULL;
    uint64_t a = k0 * k1;
    a = (a ^ (a >> 47)) * k1;                                  // ShiftMix(seed.lo * k1) * k1
    uint64_t c = k1 * k1 + ch_mix16(4u + ((uint64_t)id << 3), (uint64_t)id);  // HashLen0to16(len 4)
    uint64_t d = (a + c) ^ ((a + c) >> 47);                    // ShiftMix(a + c), len < 8
    uint64_t aa = ch_mix16(a, c);
    uint64_t bb = ch_mix16(d, k1);
    first = aa ^ bb;
    second = ch_mix16(bb, aa);
}

__global__ void k_hash_ids(const uint32_t *__restrict__ ids, uint64_t *__restrict__ out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t f, s;
    cityhash128_u32(ids[i], f, s);
    out[i] = s;
}

// ------------------------------------------------------------------ populate
struct PopArgs {
    uint64_t *first;      // [p] CityHash .first of id n-1-p
    uint64_t *second;     // [p] .second
    uint32_t *bkt_keys;   // [p] bucket
    uint32_t *pos;        // [p] = p
    int64_t n;
};

__global__ void k_pop_hash(PopArgs a, uint64_t bkt_mask)
{
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    uint32_t id = (uint32_t)(a.n - 1 - p);
    uint64_t f, s;
    cityhash128_u32(id, f, s);
    a.first[p] = f;
    a.second[p] = s;
    a.bkt_keys[p] = (uint32_t)((s & 0xFFFFFFFFu) & bkt_mask);  // mica_insert_one: 32-bit bkt field
    a.pos[p] = (uint32_t)p;
}

struct LogPlan {          // virtual offset of insert p (see hkv_runtime.hip: plan_log)
    uint64_t h0;          // head before the first insert
    uint64_t k;           // inserts before the single wrap
    uint64_t hw;          // head right after the wrap
    uint32_t e;           // entry size
};

__device__ __forceinline__ uint64_t plan_off(const LogPlan &L, uint64_t p)
{
    return p < L.k ? L.h0 + p * L.e : L.hw + (p - L.k) * L.e;
}

// one owner lane per bucket replays mica_insert_one (mica.c:78-146) for that bucket's inserts, starting from the
// bucket as it is in memory. Insert p's tag is that of key[p], its offset plan_off(L, p). The sort is stable, so a
// bucket's inserts arrive in the order of p. COUNT (the upsert; a populate's instance is the code it was): also
// counts[0] += inserts that took an in-use slot by tag match, counts[1] += evictions.
template <bool COUNT>
__global__ void k_pop_buckets(const uint32_t *__restrict__ sk, const uint32_t *__restrict__ sp,
                              const uint64_t *__restrict__ key, uint8_t *index, int64_t n,
                              LogPlan L, unsigned long long *evictions, unsigned long long *counts)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    uint32_t bkt = sk[q];
    if (q > 0 && sk[q - 1] == bkt) return;
    uint64_t *slots = reinterpret_cast<uint64_t *>(index + (uint64_t)bkt * 64u);
    uint64_t s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = slots[j];
    unsigned long long ev = 0, rep = 0;
    for (int64_t r = q; r < n && sk[r] == bkt; ++r) {
        uint32_t p = sp[r];
        uint32_t tag = (uint32_t)(key[p] >> 48);
        int use = -1;
        bool taken = false;   // the chosen slot was in use
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (slot_tag(s[j]) == tag || !slot_in_use(s[j])) {
                use = j;
                if (COUNT) taken = slot_in_use(s[j]);
            }
        if (use < 0) {
            use = (int)(tag & 7u);
            ++ev;
        }
        if (COUNT) rep += taken;
        uint64_t v = 1u | ((uint64_t)tag << 1) | (plan_off(L, p) << 24);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j == use) s[j] = v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) slots[j] = s[j];
    if (ev) atomicAdd(evictions, ev);
    if (COUNT) {
        if (rep) atomicAdd(&counts[0], rep);
        if (ev) atomicAdd(&counts[1], ev);
    }
}

// entry image of spacetime_populate_fixed_len (spacetime.c:32-68); meta fields the reference
// leaves uninitialised (ack_bv, RMW_flag, last_local_write_ts) are written as zero
__global__ void k_pop_log(const uint64_t *__restrict__ first, const uint64_t *__restrict__ second,
                          uint8_t *log, int64_t p_begin, int64_t p_end, int64_t n, LogPlan L,
                          uint64_t log_mask, uint8_t val_len_byte)
{
    int64_t p = p_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= p_end) return;
    uint64_t id = (uint64_t)(n - 1 - p);
    uint64_t *e = reinterpret_cast<uint64_t *>(log + (plan_off(L, (uint64_t)p) & log_mask));
    uint64_t vv = 0x0101010101010101ULL * (uint8_t)('a' + (id % 20));
    e[0] = first[p];
    e[1] = second[p];
    // bytes 16..23: opcode PUT, val_len, state VALID, ack_bv 0, lwid 127, obi 255, lock 0, cid 255
    e[2] = (uint64_t)kOpPut | ((uint64_t)val_len_byte << 8) | ((uint64_t)kValid << 16) |
           ((uint64_t)(kLwidEmpty << 1) << 32) | ((uint64_t)kObiEmpty << 40) | ((uint64_t)kCidEmpty << 56);
    e[3] = 0;                      // ts.version, llw cid, llw version (low bytes)
    e[4] = vv & ~0xFFULL;          // llw version top byte, value from byte 33
    for (uint32_t w = 5; w < L.e / 8; ++w) e[w] = vv;
}

// ------------------------------------------------------------------ host-side launchers
int launch_hash_ids(const uint32_t *ids, uint64_t *out, int64_t n, hipStream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_hash_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, out, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Stable LSD radix sort of (bucket, insert) pairs. rocPRIM picks a merge sort below 1M
// items by default; a merge_sort_limit of 0 keeps every size on the Onesweep radix passes
// (ceil(key_bits / 8) passes over 8-byte pairs), which is what the key width makes cheapest.
// Onesweep with 10-bit digits (3 passes for the 28-bit entry ids of a 100M-key table) and
// 1024x8 tiles: measured fastest on gfx950 for 0.8M-8M pairs (tools/sort_bench.hip,
// profiles/r01_sort_configs.txt); rocPRIM's default (1024x16, 8-bit) is 20-30% slower here.
using SortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<1024, 8>, 10,
                                        rocprim::block_radix_rank_algorithm::match>,
    0>;

size_t sort_temp_bytes(int64_t n, int key_bits)
{
    size_t bytes = 0;
    rocprim::radix_sort_pairs<SortConfig>(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                          (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u,
                                          (unsigned)key_bits);
    return bytes;
}

int sort_pairs(void *tmp, size_t tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
               uint32_t *vout, int64_t n, int key_bits, hipStream_t s)
{
    hipError_t e = rocprim::radix_sort_pairs<SortConfig>(tmp, tmp_bytes, kin, kout, vin, vout, (size_t)n, 0u,
                                                         (unsigned)key_bits, s);
    return e == hipSuccess ? 0 : -1;
}

int launch_populate(const PopulateLaunch &pl, hipStream_t s)
{
    const int64_t n = pl.n;
    if (n <= 0) return 0;
    const unsigned grid = (unsigned)((n + 255) / 256);
    PopArgs a{pl.first, pl.second, pl.keys_a, pl.vals_a, n};
    hipLaunchKernelGGL(k_pop_hash, dim3(grid), dim3(256), 0, s, a, pl.bkt_mask);
    if (hipGetLastError() != hipSuccess) return -1;
    if (sort_pairs(pl.sort_tmp, pl.sort_tmp_bytes, pl.keys_a, pl.keys_b, pl.vals_a, pl.vals_b, n, pl.key_bits, s))
        return -2;
    LogPlan L{pl.h0, pl.k, pl.hw, pl.entry_size};
    hipLaunchKernelGGL(k_pop_buckets<false>, dim3(grid), dim3(256), 0, s, pl.keys_b, pl.vals_b, pl.second, pl.index, n,
                       L, pl.evictions, (unsigned long long *)nullptr);
    if (hipGetLastError() != hipSuccess) return -3;
    // later inserts overwrite earlier ones when the log wraps: write in chunks no longer than one
    // physical lap, in insertion order
    // (a run of inserts never overlaps itself physically while it stays within one lap of the
    // log and does not cross the single wrap point, so each launch covers such a run)
    int64_t chunk = (int64_t)(pl.log_cap / pl.entry_size);
    if (chunk < 1) chunk = 1;
    const int64_t wrap_at = pl.k < (uint64_t)n ? (int64_t)pl.k : n;
    const int64_t runs[2][2] = {{0, wrap_at}, {wrap_at, n}};
    for (const auto &r : runs) {
        for (int64_t b = r[0]; b < r[1]; b += chunk) {
            int64_t e = b + chunk < r[1] ? b + chunk : r[1];
            hipLaunchKernelGGL(k_pop_log, dim3((unsigned)((e - b + 255) / 256)), dim3(256), 0, s, pl.first,
                               pl.second, pl.log, b, e, n, L, pl.log_mask, pl.val_len_byte);
            if (hipGetLastError() != hipSuccess) return -4;
        }
    }
    return 0;
}

// ------------------------------------------------------------------ the inline residency's conversions
// Four lanes per bucket, 16 B each (two slots). The inline key is the one in the bucket's lowest in-use slot:
// chosen from the bucket alone, so the same key whenever the conversion runs (nothing is inserted under the
// rounds). to_inline copies the bucket into the first half of its line with that slot flagged and the key's
// whole 64-B entry into the second half; to_log copies the second half back to the entry's log offset. An
// empty bucket's line holds the (empty) bucket and no flag; its second half is never read.
template <bool TO_INLINE>
__global__ __launch_bounds__(256) void k_layout_convert(const uint8_t *index, uint8_t *log, uint8_t *line,
                                                        uint64_t num_bkts, uint64_t log_mask)
{
    const int q = threadIdx.x & 3, gbase = (threadIdx.x & 63) & ~3;
    const uint64_t b = (uint64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    const bool live = b < num_bkts;   // (the four lanes of a group share b: a group is live or idle as a whole)
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (live) v = bucket_words(index, b)[q];
    const uint64_t s0 = u64_of(v.x, v.y), s1 = u64_of(v.z, v.w);
    const uint32_t o = group_slots(live && slot_in_use(s0), live && slot_in_use(s1), gbase);   // the slots in use
    const int first = o ? __ffs(o) - 1 : 0;
    const uint64_t off = group_slot_word(slot_off_raw(s0), slot_off_raw(s1), first);
    if (!live) return;
    uint4 *ln = line_words(line, b);
    uint4 *ent = reinterpret_cast<uint4 *>(log + (off & log_mask));
    if (TO_INLINE) {
        if (o && (first >> 1) == q) {
            if (first & 1) v.w |= (uint32_t)(kInlineSlotBit >> 32);
            else v.y |= (uint32_t)(kInlineSlotBit >> 32);
        }
        ln[q] = v;
        ln[4 + q] = o ? ent[q] : make_uint4(0u, 0u, 0u, 0u);
    } else if (o) {
        ent[q] = ln[4 + q];
    }
}

int launch_layout_convert(const uint8_t *index, uint8_t *log, uint8_t *line, uint64_t num_bkts, uint64_t log_mask,
                          bool to_inline, hipStream_t s)
{
    const unsigned grid = (unsigned)((num_bkts + 63) / 64);
    if (to_inline) hipLaunchKernelGGL(k_layout_convert<true>, dim3(grid), dim3(256), 0, s, index, log, line, num_bkts, log_mask);
    else hipLaunchKernelGGL(k_layout_convert<false>, dim3(grid), dim3(256), 0, s, index, log, line, num_bkts, log_mask);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------ the table census
// hermeskv.h "Table census and digest". A streaming pass over the buckets like the conversions: four lanes per
// bucket, 16 B each, 64 buckets per block and step, a grid of a few blocks per CU striding over the table. IL
// reads the 128-B lines (the bucket, and the inline key's entry from the line's second half -- its log entry
// is stale), else the 64-B buckets; every other live slot's entry comes from the log, 64 B per step of the
// lane group. A lane hashes the two words it holds of each 64 B (the position salt makes that independent of
// the other lanes) and the group adds up. Lane 1 of a group holds state, op_buffer_index and timestamp (entry
// words 2 and 3) and keeps the group's counts. Every count is reduced per wave by shuffles and per block through
// LDS, then one atomic per field and block goes to memory: tens of thousands for the whole table, and sums,
// xors and maxima only, so the result is the same bytes in whatever order they land.
namespace {
constexpr uint64_t kMixG = 0x9E3779B97F4A7C15ull;
// word indices of hkv_census
enum : int { kCsKeys = 0, kCsDead = 1, kCsState = 2, kCsObi = 10, kCsCid = 11, kCsMaxTs = 20, kCsSum = 21,
             kCsXor = 22, kCsLines = 23, kCsOffenders = 24 };
static_assert(kCsOffenders + 1 == kCensusWords, "hkv_census is kCensusWords 64-bit words");
constexpr int kCensusBlock = 256;                 // threads: 64 buckets per step
constexpr int kCensusBktsPerBlock = kCensusBlock / 4;

__device__ __forceinline__ uint64_t mix64(uint64_t x)   // the splitmix64 finaliser
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// N per-thread values -> out[0..N): per wave by shuffles, per block through LDS, then one atomic per non-zero field
// and block (0 is neutral). Field KMAX combines by max, KXOR by xor (-1: none), the rest by add. Every thread calls it.
template <int KMAX = -1, int KXOR = -1, class T, int N>
__device__ __forceinline__ void block_reduce(const T (&v)[N], unsigned long long *out)
{
    using U = unsigned long long;
    const auto red_op = [](int k, U x, U y) { return k == KMAX ? (y > x ? y : x) : k == KXOR ? x ^ y : x + y; };
    __shared__ unsigned long long sh[kCensusBlock / 64][N];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        unsigned long long x = v[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x = red_op(k, x, __shfl_xor(x, d));
        if (lane == 0) sh[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        unsigned long long x = sh[0][k];
        for (int w = 1; w < kCensusBlock / 64; ++w) x = red_op(k, x, sh[w][k]);
        if (x) {
            if (k == KMAX) atomicMax(&out[k], x);
            else if (k == KXOR) atomicXor(&out[k], x);
            else atomicAdd(&out[k], x);
        }
    }
}

// The digest's h (hermeskv.h "Table census and digest") of the entry whose first 64 B the group of four lanes
// holds -- lane q its words 2q (wa) and 2q + 1 (wb) -- and whose further 64-B runs (BIG) follow at ent: a lane
// hashes the words it holds (the position salt makes that independent of the other lanes), the group adds up.
// The same h in all four lanes.
template <bool BIG>
__device__ __forceinline__ uint64_t entry_hash(uint64_t wa, uint64_t wb, const uint4 *ent, int q, uint32_t chunks,
                                               uint64_t mask_a, uint64_t mask_b)
{
    uint64_t e = mix64((wb & mask_b) + (uint64_t)(2 * q + 2) * kMixG);
    if (q) e += mix64((wa & mask_a) + (uint64_t)(2 * q + 1) * kMixG);   // (word 0 is skipped)
    if (BIG) {
        for (uint32_t k = 1; k < chunks; ++k) {
            const uint4 d = ent[4 * k + q];
            const uint64_t i = 8ull * k + 2u * q;
            e += mix64(u64_of(d.x, d.y) + (i + 1) * kMixG) + mix64(u64_of(d.z, d.w) + (i + 2) * kMixG);
        }
    }
    e += __shfl_xor(e, 1, 4);
    e += __shfl_xor(e, 2, 4);
    return mix64(e);
}

// The passes' persistent grid: as many blocks per CU as the kernel's registers let a CU hold at once (at most cap;
// fn NULL: cap itself), so the blocks all start and end together -- a grid that needs a second, partial round of
// blocks ends with idle CUs. No block waits for another, so any grid gives the same result.
dim3 persistent_grid(const void *fn, uint64_t items, uint64_t items_per_step, int device, int cap)
{
    int cus = 0, bpc = cap;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    if (fn && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, fn, kCensusBlock, 0) != hipSuccess || bpc <= 0)) bpc = 4;
    if (bpc > cap) bpc = cap;
    const uint64_t steps = (items + items_per_step - 1) / items_per_step, most = (uint64_t)cus * bpc;
    return dim3((unsigned)(steps < most ? steps : most));
}

// f(IL, BIG) as two std::bool_constants for a pass's instance: the inline residency's lines (never with big
// entries), or index and log with entries of 64 B or more
template <class F>
void with_instance(bool il, bool big, F &&f)
{
    if (il) f(std::true_type{}, std::false_type{});
    else if (big) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}
}  // namespace

template <bool IL, bool BIG>
__global__ __launch_bounds__(kCensusBlock) void k_table_census(const uint8_t *__restrict__ index,
                                                               const uint8_t *__restrict__ log,
                                                               const uint8_t *__restrict__ line, uint64_t num_bkts,
                                                               uint64_t log_mask, uint64_t log_head, uint64_t log_cap,
                                                               uint32_t chunks, unsigned long long *out,
                                                               unsigned long long *offender_keys, uint64_t offender_cap)
{
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63, gbase = lane & ~3;
    const uint64_t tiles = (num_bkts + kCensusBktsPerBlock - 1) / kCensusBktsPerBlock;
    uint32_t n_keys = 0, n_dead = 0, n_obi = 0, n_lines = 0, n_off = 0, n_state[6] = {0, 0, 0, 0, 0, 0},
             n_cid[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t max_ts = 0, dsum = 0, dxor = 0;
    const uint64_t mask_a = digest_mask_a(q), mask_b = digest_mask_b(q);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform)
        const uint64_t b = tile * kCensusBktsPerBlock + (threadIdx.x >> 2);
        const bool live = b < num_bkts;   // (the four lanes of a group share b)
        uint4 v = make_uint4(0u, 0u, 0u, 0u), iv = v;
        if (live) {
            const uint4 *src = IL ? line_words(line, b) : bucket_words(index, b);
            v = src[q];
            if (IL) iv = src[4 + q];
        }
        const uint64_t s0 = u64_of(v.x, v.y), s1 = u64_of(v.z, v.w);
        uint32_t o = group_slots(live && slot_in_use(s0), live && slot_in_use(s1), gbase);   // the slots in use
        while (o) {   // (group-uniform: the four lanes of a group stay together)
            const int j = __ffs(o) - 1;
            o &= o - 1;
            const uint64_t raw = slot_off_raw(group_slot_word(s0, s1, j)), off = off_of<IL>(raw);
            const bool il = off_is_inline<IL>(raw);
            if (!in_log_window(log_head, log_cap, off)) {   // the log has overwritten the entry
                ++n_dead;
                continue;
            }
            const uint4 *ent = reinterpret_cast<const uint4 *>(log + (off & log_mask));
            const uint4 c = il ? iv : ent[q];
            const uint64_t wa = u64_of(c.x, c.y), wb = u64_of(c.z, c.w);
            const uint64_t h = entry_hash<BIG>(wa, wb, ent, q, chunks, mask_a, mask_b);
            const uint64_t key = __shfl(wb, 0, 4);
            // lane 1: wa = entry bytes 16..23, wb = 24..31
            const uint32_t state = (uint32_t)(wa >> 16) & 0xFFu, obi = (uint32_t)(wa >> 40) & 0xFFu,
                           cid = (uint32_t)(wa >> 56);
            const uint64_t ts = ((wb & 0xFFFFFFFFull) << 8) | cid;
            const bool not_valid = state != kValid;
            const uint32_t si = state >= 1 && state <= 5 ? state : 0, ci = cid < 8 ? cid : 8;
            ++n_keys;
            n_lines += il;
            n_obi += obi != kObiEmpty;
#pragma unroll
            for (int k = 0; k < 6; ++k) n_state[k] += si == (uint32_t)k;
#pragma unroll
            for (int k = 0; k < 9; ++k) n_cid[k] += not_valid && ci == (uint32_t)k;
            max_ts = ts > max_ts ? ts : max_ts;
            dsum += h;
            dxor ^= mix64(h + kMixG);
            if (offender_keys) {   // (uniform) one returning atomic per wave and step that found offenders
                const bool mine = q == 1 && not_valid;
                const unsigned long long m = __ballot(mine);
                if (m) {
                    const int leader = __ffsll(m) - 1;
                    unsigned long long base = 0;
                    if (lane == leader) base = atomicAdd(&out[kCsOffenders], (unsigned long long)__popcll(m));
                    base = __shfl(base, leader);
                    const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1));
                    if (mine && pos < offender_cap) offender_keys[pos] = key;
                }
            } else {
                n_off += not_valid;
            }
        }
    }
    // only lane 1 of a group read the meta: its counts are the group's
    unsigned long long r[kCensusWords];
#pragma unroll
    for (int k = 0; k < kCensusWords; ++k) r[k] = 0;
    if (q == 1) {
        r[kCsKeys] = n_keys;
        r[kCsDead] = n_dead;
#pragma unroll
        for (int k = 0; k < 6; ++k) r[kCsState + k] = n_state[k];
        r[kCsObi] = n_obi;
#pragma unroll
        for (int k = 0; k < 9; ++k) r[kCsCid + k] = n_cid[k];
        r[kCsMaxTs] = max_ts;
        r[kCsSum] = dsum;
        r[kCsXor] = dxor;
        r[kCsLines] = n_lines;
        r[kCsOffenders] = n_off;
    }
    block_reduce<kCsMaxTs, kCsXor>(r, out);
}

int launch_table_census(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                        uint64_t num_bkts, unsigned long long *out, unsigned long long *offender_keys,
                        uint64_t offender_cap, int device, hipStream_t s)
{
    if (g.entry_size % 64 || (line && g.entry_size != 64)) return -1;
    if (hipMemsetAsync(out, 0, kCensusWords * sizeof(unsigned long long), s) != hipSuccess) return -2;
    const uint32_t chunks = g.entry_size / 64;
    // HKV_CENSUS_BLOCKS_PER_CU sets the grid's blocks per CU instead of the occupancy query (timing experiments)
    static const int env_bpc = getenv("HKV_CENSUS_BLOCKS_PER_CU") ? atoi(getenv("HKV_CENSUS_BLOCKS_PER_CU")) : 0;
    if (!offender_cap) offender_keys = nullptr;
    with_instance(line != nullptr, chunks > 1, [&](auto il, auto big) {
        const auto k = k_table_census<decltype(il)::value, decltype(big)::value>;
        // with the override there is no occupancy query (fn NULL) and the cap is the blocks per CU, at most 8
        const dim3 grid = persistent_grid(env_bpc > 0 ? nullptr : (const void *)k, num_bkts, kCensusBktsPerBlock, device,
                                          env_bpc > 0 && env_bpc < 8 ? env_bpc : 8);
        hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, index, log, line, num_bkts, g.log_mask, g.log_head, g.log_cap, chunks, out, offender_keys,
                           offender_cap);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------ the partitioned census
// hermeskv.h "Partitioned census and delta repair": the census's digest_sum, digest_xor, keys and offenders per
// partition p = key & (P - 1), P = 2^part_bits <= num_bkts, which is b & (P - 1) for every key of bucket b. Four
// lanes per bucket with the census's loads and its liveness and residency rules (part_bucket below is that loop
// with four sums); a row is four 64-bit words {sum, xor, keys, not VALID}. One atomic per bucket and field would
// be 2^27 x 3 or 4 of them for the 100M-key table against ~22 G/s, so the sums have to meet on chip.
//
// Mapping A (k_table_census_parts, the default). A group of four lanes owns one partition for a whole unit of
// work and walks the buckets b, b + S, b + 2S, ... with S = max(P, 64): they all lie in its partition, the sums
// stay in registers, and a block step still reads 64 consecutive buckets. A unit is (a tile of 64 partitions, one
// of `splits` pieces of the stride range); the blocks stride over the units. With P >= 64 and splits == 1 a row
// has one owner, who writes it with two plain 16-B stores (lane 0: sum, xor; lane 1: keys, not VALID) -- no atomic
// and no memset. Otherwise (P < 64: groups P apart share a partition; or too few tiles to fill the grid, so the
// stride range is split over blocks) the groups add up per partition in LDS and the block sends at most four
// atomics per partition and unit to rows the launch zeroed first.
// Mapping B (k_table_census_parts_b, HKV_CENSUS_PARTS_MAPPING=B; kept for tools/delta_bench.py, which times it
// beside A). The census's contiguous order. With P < 64 a group's partition is the same at every step, so it is
// A's atomic path; with P >= 64 no two buckets of a step share a partition and every bucket's non-zero fields go
// to the rows as atomics, one field per lane.
// Measured (profiles/delta_100m.txt, 100M keys in 2^27 buckets, part_bits 12 / 16 / 20): A 6.10 / 6.14 / 6.12 ms
// on a LOG table and 5.70 / 5.64 / 5.66 ms on an INLINE one, B 6.57 / 6.51 / 6.65 and 6.01 / 6.18 / 6.19 ms, the
// census itself 7.69 and 7.82 ms in that session. A is faster at every size, its stride of 64 P bytes per step
// (64 MiB at part_bits 20) costs nothing that shows, so A is the default.
// Every field is a sum or an xor: any mapping, grid or split gives the same bytes.
namespace {
constexpr int kPartWords = 4;   // sizeof(hkv_part_row) / 8

// bucket b's live keys into the group's sums: dsum, dxor and n_keys in all four lanes, n_nv in lane 1 (which
// holds the state byte). live: b is a bucket of the table (the four lanes of a group share it).
template <bool IL, bool BIG>
__device__ __forceinline__ void part_bucket(const uint8_t *__restrict__ index, const uint8_t *__restrict__ log,
                                            const uint8_t *__restrict__ line, uint64_t b, bool live, int q, int gbase,
                                            uint64_t log_mask, uint64_t log_head, uint64_t log_cap, uint32_t chunks,
                                            uint64_t mask_a, uint64_t mask_b, uint64_t &dsum, uint64_t &dxor,
                                            uint32_t &n_keys, uint32_t &n_nv)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u), iv = v;
    if (live) {
        const uint4 *src = IL ? line_words(line, b) : bucket_words(index, b);
        v = src[q];
        if (IL) iv = src[4 + q];
    }
    const uint64_t s0 = u64_of(v.x, v.y), s1 = u64_of(v.z, v.w);
    uint32_t o = group_slots(live && slot_in_use(s0), live && slot_in_use(s1), gbase);   // the slots in use
    while (o) {   // (group-uniform)
        const int j = __ffs(o) - 1;
        o &= o - 1;
        const uint64_t raw = slot_off_raw(group_slot_word(s0, s1, j)), off = off_of<IL>(raw);
        if (!in_log_window(log_head, log_cap, off)) continue;   // the log has overwritten the entry
        const uint4 *ent = reinterpret_cast<const uint4 *>(log + (off & log_mask));
        const uint4 c = off_is_inline<IL>(raw) ? iv : ent[q];
        const uint64_t wa = u64_of(c.x, c.y), wb = u64_of(c.z, c.w);
        const uint64_t h = entry_hash<BIG>(wa, wb, ent, q, chunks, mask_a, mask_b);
        ++n_keys;
        n_nv += ((uint32_t)(wa >> 16) & 0xFFu) != kValid;   // lane 1: wa = entry bytes 16..23
        dsum += h;
        dxor ^= mix64(h + kMixG);
    }
}

// The groups' sums of one unit, added up per partition in LDS (group gi's partition is slot gi & slot_mask of
// sh), then at most four atomics per slot to rows[row0 + slot]. Every thread of the block calls it.
__device__ __forceinline__ void part_rows_combine(unsigned long long (&sh)[kCensusBktsPerBlock * kPartWords], int q,
                                                  uint32_t slot_mask, uint64_t dsum, uint64_t dxor, uint32_t n_keys,
                                                  uint32_t n_nv, unsigned long long *rows, uint64_t row0)
{
    const uint32_t t = threadIdx.x;   // kCensusBlock threads: one per word of sh
    sh[t] = 0;
    __syncthreads();
    if (q == 1 && n_keys) {
        unsigned long long *r = sh + ((t >> 2) & slot_mask) * kPartWords;
        atomicAdd(r + 0, (unsigned long long)dsum);
        atomicXor(r + 1, (unsigned long long)dxor);
        atomicAdd(r + 2, (unsigned long long)n_keys);
        if (n_nv) atomicAdd(r + 3, (unsigned long long)n_nv);
    }
    __syncthreads();
    // (thread t reads the word it zeroes at the next call: no barrier between the two is needed)
    const unsigned long long x = sh[t];
    if ((t >> 2) <= slot_mask && x) {
        unsigned long long *dst = rows + (row0 + (t >> 2)) * kPartWords + (t & 3);
        if ((t & 3) == 1) atomicXor(dst, x);
        else atomicAdd(dst, x);
    }
}
}  // namespace

template <bool IL, bool BIG>
__global__ __launch_bounds__(kCensusBlock) void k_table_census_parts(const uint8_t *__restrict__ index,
                                                                     const uint8_t *__restrict__ log,
                                                                     const uint8_t *__restrict__ line,
                                                                     uint64_t num_bkts, uint64_t log_mask,
                                                                     uint64_t log_head, uint64_t log_cap,
                                                                     uint32_t chunks, uint32_t part_bits,
                                                                     uint32_t splits, unsigned long long *rows)
{
    const int q = threadIdx.x & 3, gbase = (threadIdx.x & 63) & ~3;
    const uint32_t gi = threadIdx.x >> 2;
    const uint64_t P = 1ull << part_bits, S = P > kCensusBktsPerBlock ? P : (uint64_t)kCensusBktsPerBlock;
    const uint64_t ptiles = S / kCensusBktsPerBlock, K = (num_bkts + S - 1) / S, units = ptiles * splits;
    const bool owner = P >= kCensusBktsPerBlock && splits == 1;   // (uniform) every row has one group
    const uint64_t mask_a = digest_mask_a(q), mask_b = digest_mask_b(q);
    __shared__ unsigned long long sh[kCensusBktsPerBlock * kPartWords];
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {   // (block-uniform)
        const uint64_t pt = u % ptiles, sp = u / ptiles;
        const uint64_t k0 = K * sp / splits, k1 = K * (sp + 1) / splits;
        const uint64_t first = pt * kCensusBktsPerBlock + gi;   // < S: the group's partition is first & (P - 1)
        uint64_t dsum = 0, dxor = 0;
        uint32_t n_keys = 0, n_nv = 0;   // (at most 8 (k1 - k0) <= num_bkts / 8 keys)
        for (uint64_t k = k0; k < k1; ++k) {
            const uint64_t b = first + k * S;
            part_bucket<IL, BIG>(index, log, line, b, b < num_bkts, q, gbase, log_mask, log_head, log_cap, chunks,
                                 mask_a, mask_b, dsum, dxor, n_keys, n_nv);
        }
        if (owner) {   // S == P and num_bkts is a multiple of it: first < P is a partition, and this group's alone
            n_nv = __shfl(n_nv, 1, 4);
            uint4 *row = reinterpret_cast<uint4 *>(rows + first * kPartWords);
            if (q == 0) row[0] = make_uint4((uint32_t)dsum, (uint32_t)(dsum >> 32), (uint32_t)dxor, (uint32_t)(dxor >> 32));
            if (q == 1) row[1] = make_uint4(n_keys, 0u, n_nv, 0u);
        } else {
            part_rows_combine(sh, q, (uint32_t)((P < kCensusBktsPerBlock ? P : (uint64_t)kCensusBktsPerBlock) - 1), dsum, dxor,
                              n_keys, n_nv, rows, P < kCensusBktsPerBlock ? 0 : pt * kCensusBktsPerBlock);
        }
    }
}

template <bool IL, bool BIG>
__global__ __launch_bounds__(kCensusBlock) void k_table_census_parts_b(const uint8_t *__restrict__ index,
                                                                       const uint8_t *__restrict__ log,
                                                                       const uint8_t *__restrict__ line,
                                                                       uint64_t num_bkts, uint64_t log_mask,
                                                                       uint64_t log_head, uint64_t log_cap,
                                                                       uint32_t chunks, uint32_t part_bits,
                                                                       unsigned long long *rows)
{
    const int q = threadIdx.x & 3, gbase = (threadIdx.x & 63) & ~3;
    const uint64_t P = 1ull << part_bits;
    const bool shared = P < kCensusBktsPerBlock;   // (uniform) a group's partition is the same at every step
    const uint64_t tiles = (num_bkts + kCensusBktsPerBlock - 1) / kCensusBktsPerBlock;
    const uint64_t mask_a = digest_mask_a(q), mask_b = digest_mask_b(q);
    __shared__ unsigned long long sh[kCensusBktsPerBlock * kPartWords];
    uint64_t dsum = 0, dxor = 0;
    uint32_t n_keys = 0, n_nv = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform)
        const uint64_t b = tile * kCensusBktsPerBlock + (threadIdx.x >> 2);
        part_bucket<IL, BIG>(index, log, line, b, b < num_bkts, q, gbase, log_mask, log_head, log_cap, chunks, mask_a,
                             mask_b, dsum, dxor, n_keys, n_nv);
        if (shared) continue;
        n_nv = __shfl(n_nv, 1, 4);
        const unsigned long long x = q == 0 ? dsum : q == 1 ? dxor : q == 2 ? n_keys : n_nv;   // a field per lane
        if (x) {
            unsigned long long *dst = rows + (b & (P - 1)) * kPartWords + q;
            if (q == 1) atomicXor(dst, x);
            else atomicAdd(dst, x);
        }
        dsum = dxor = 0;
        n_keys = n_nv = 0;
    }
    if (shared) part_rows_combine(sh, q, (uint32_t)(P - 1), dsum, dxor, n_keys, n_nv, rows, 0);
}

int launch_table_census_parts(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                              uint64_t num_bkts, uint32_t part_bits, unsigned long long *rows, int device, hipStream_t s)
{
    const uint64_t P = 1ull << part_bits;
    if (g.entry_size % 64 || (line && g.entry_size != 64) || part_bits > 63 || P > num_bkts) return -1;
    const uint32_t chunks = g.entry_size / 64;
    const char *env = getenv("HKV_CENSUS_PARTS_MAPPING");   // (read at every call: a tool times both in one process)
    const bool map_b = env && (env[0] == 'B' || env[0] == 'b');
    hipError_t zeroed = hipSuccess;
    with_instance(line != nullptr, chunks > 1, [&](auto il, auto big) {
        constexpr bool IL = decltype(il)::value, BIG = decltype(big)::value;
        if (map_b) {
            const auto k = k_table_census_parts_b<IL, BIG>;
            zeroed = hipMemsetAsync(rows, 0, P * kPartWords * sizeof(unsigned long long), s);
            if (zeroed != hipSuccess) return;
            const dim3 grid = persistent_grid((const void *)k, num_bkts, kCensusBktsPerBlock, device, 8);
            hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, index, log, line, num_bkts, g.log_mask, g.log_head, g.log_cap, chunks, part_bits, rows);
            return;
        }
        const auto k = k_table_census_parts<IL, BIG>;
        // the blocks the census would run on this table: what the units have to fill
        const uint64_t full = persistent_grid((const void *)k, num_bkts, kCensusBktsPerBlock, device, 8).x;
        const uint64_t S = P > kCensusBktsPerBlock ? P : (uint64_t)kCensusBktsPerBlock;
        const uint64_t ptiles = S / kCensusBktsPerBlock, K = (num_bkts + S - 1) / S;
        uint64_t splits = ptiles >= full ? 1 : (full + ptiles - 1) / ptiles;
        if (splits > K) splits = K;
        if (P < kCensusBktsPerBlock || splits > 1) {   // the rows are added to
            zeroed = hipMemsetAsync(rows, 0, P * kPartWords * sizeof(unsigned long long), s);
            if (zeroed != hipSuccess) return;
        }
        const uint64_t units = ptiles * splits;
        hipLaunchKernelGGL(k, dim3((unsigned)(units < full ? units : full)), dim3(kCensusBlock), 0, s, index, log, line, num_bkts, g.log_mask, g.log_head,
                           g.log_cap, chunks, part_bits, (uint32_t)splits, rows);
    });
    if (zeroed != hipSuccess) return -2;
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// d_mask[p] = the two rows differ (accumulate: or-ed into the byte that is there); count = the non-zero bytes
// afterwards: one streaming pass, a thread per row, one atomic per block
__global__ __launch_bounds__(kCensusBlock) void k_part_rows_diff(const uint4 *__restrict__ a, const uint4 *__restrict__ b,
                                                                 uint64_t P, uint8_t *mask, unsigned long long *count,
                                                                 int accumulate)
{
    uint32_t n[1] = {0};
    for (uint64_t p = (uint64_t)blockIdx.x * kCensusBlock + threadIdx.x; p < P; p += (uint64_t)gridDim.x * kCensusBlock) {
        const uint4 a0 = a[2 * p], a1 = a[2 * p + 1], b0 = b[2 * p], b1 = b[2 * p + 1];
        const bool differ = ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) |
                             (a1.z ^ b1.z) | (a1.w ^ b1.w)) != 0;
        const uint8_t m = (uint8_t)((accumulate ? mask[p] : 0) | (differ ? 1 : 0));
        mask[p] = m;
        n[0] += m != 0;
    }
    block_reduce(n, count);
}

int launch_part_rows_diff(const void *a, const void *b, uint32_t part_bits, uint8_t *mask, unsigned long long *count,
                          int accumulate, int device, hipStream_t s)
{
    if (part_bits > 63) return -1;
    const uint64_t P = 1ull << part_bits;
    if (hipMemsetAsync(count, 0, sizeof(unsigned long long), s) != hipSuccess) return -2;
    const dim3 grid = persistent_grid(nullptr, P, kCensusBlock, device, 8);
    hipLaunchKernelGGL(k_part_rows_diff, grid, dim3(kCensusBlock), 0, s, static_cast<const uint4 *>(a), static_cast<const uint4 *>(b), P, mask, count,
                       accumulate);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------ replica repair: extract and install
// hermeskv.h "Replica repair". A record is the entry image under the digest's mask, so both kernels move entries
// as the 16-B chunks the census reads: lane q of a group of four holds bytes 16q..16q+15 of an entry's first 64 B
// (q = 1: the meta -- state, ts cid, ts version; q = 2, 3: the value from byte 33 on), and a 320-B entry's other
// 256 B are value only.
// The census's pass over the buckets [bkt_lo, bkt_hi): every live slot whose timestamp is at least min_ts leaves
// as one record. A block step takes kExtractK buckets per group of four lanes (512 per block) in three parts:
// count (which slots qualify -- from the buckets alone when min_ts is 0, else with each entry's meta), reserve
// (a prefix sum over the block and ONE returning atomic on the record counter, result[0]), write (each record as
// whole 64-B runs, 16 B per lane, the mask applied in registers; nothing at or past record_cap). One atomic per
// wave and step, as the census's offender list takes, was measured first: every one of them lands on the same
// address, about 25M of them for 100M keys, and the extract took 258 ms (profiles/repair_100m.txt).
// MASKED (hkv_table_extract_parts_async): a bucket whose partition b & part_mask_of has a zero byte in part_sel is
// not loaded and counts nowhere -- its words stay zero, as an idle group's. The selection bytes, 2 MiB at most,
// stay in L2. A template parameter, so that the unmasked instances are the code they were.
constexpr int kExtractK = 8;
constexpr uint64_t kExtractBktsPerStep = (uint64_t)kCensusBktsPerBlock * kExtractK;   // buckets of one block step
template <bool IL, bool BIG, bool MASKED>
__global__ __launch_bounds__(kCensusBlock) void k_table_extract(const uint8_t *__restrict__ index,
                                                                const uint8_t *__restrict__ log,
                                                                const uint8_t *__restrict__ line, uint64_t bkt_lo,
                                                                uint64_t bkt_hi, uint64_t log_mask, uint64_t log_head,
                                                                uint64_t log_cap, uint32_t chunks, uint64_t min_ts,
                                                                uint4 *__restrict__ records, uint64_t record_cap,
                                                                unsigned long long *result,
                                                                const uint8_t *__restrict__ part_sel,
                                                                uint64_t part_mask_of)
{
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63, gbase = lane & ~3, wave = threadIdx.x >> 6;
    const uint64_t tiles = (bkt_hi - bkt_lo + kExtractBktsPerStep - 1) / kExtractBktsPerStep;
    __shared__ unsigned long long s_wtot[kCensusBlock / 64], s_base;
    uint32_t n_scanned[1] = {0};
    const uint64_t mask_a = digest_mask_a(q), mask_b = digest_mask_b(q);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform)
        const uint64_t b0 = bkt_lo + tile * kExtractBktsPerStep + (threadIdx.x >> 2);   // (the four lanes of a group share it)
        // count: which slots of the group's kExtractK buckets leave as records (bit 8k + j: slot j of bucket k)
        uint4 v[kExtractK];
#pragma unroll
        for (int k = 0; k < kExtractK; ++k) {
            const uint64_t b = b0 + (uint64_t)k * kCensusBktsPerBlock;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (b < bkt_hi && (!MASKED || part_sel[b & part_mask_of]))
                v[k] = (IL ? line_words(line, b) : bucket_words(index, b))[q];
        }
        uint64_t qm = 0;
#pragma unroll
        for (int k = 0; k < kExtractK; ++k) {
            const uint64_t b = b0 + (uint64_t)k * kCensusBktsPerBlock;
            const uint64_t s0 = u64_of(v[k].x, v[k].y), s1 = u64_of(v[k].z, v[k].w);
            // the live slots: in use and inside the log window; an idle group's words are zero
            uint32_t o = group_slots(slot_in_use(s0) && in_log_window(log_head, log_cap, off_of<IL>(slot_off_raw(s0))),
                                     slot_in_use(s1) && in_log_window(log_head, log_cap, off_of<IL>(slot_off_raw(s1))), gbase);
            if (q == 0) n_scanned[0] += __popc(o);
            if (min_ts) {   // (uniform) the filter needs each entry's timestamp: its bytes 16..31, the same for the four lanes
                uint32_t left = o;
                while (left) {   // (group-uniform)
                    const int j = __ffs(left) - 1;
                    left &= left - 1;
                    const uint64_t off = slot_off_raw(group_slot_word(s0, s1, j));
                    // (line_entry_of_bucket written out, here and below: through the call the <true, false>
                    // instance takes 104 VGPRs for 90 and loses a wave, profiles/table_dev_registers.txt)
                    const uint4 m = off_is_inline<IL>(off)
                                        ? reinterpret_cast<const uint4 *>(line + b * kLineBytes + kLineEntryOff)[1]
                                        : reinterpret_cast<const uint4 *>(log + (off_of<IL>(off) & log_mask))[1];
                    if ((((uint64_t)m.z << 8) | (m.y >> 24)) < min_ts) o &= ~(1u << j);
                }
            }
            qm |= (uint64_t)o << (8 * k);
        }
        // reserve: the groups' counts scanned over the wave by shuffles and over the block through LDS, then one
        // returning atomic on the record counter per block and step
        const uint32_t cnt = (uint32_t)__popcll(qm);
        uint32_t x = q == 0 ? cnt : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const uint32_t excl = (uint32_t)__shfl(x, 0, 4) - cnt;   // records of the wave's groups before this one
        const uint32_t wtot = (uint32_t)__shfl(x, 63);
        if (lane == 0) s_wtot[wave] = wtot;
        __syncthreads();
        uint64_t before = excl, total = 0;
#pragma unroll
        for (int w = 0; w < kCensusBlock / 64; ++w) {
            const uint64_t t = s_wtot[w];
            if (w < wave) before += t;
            total += t;
        }
        if (threadIdx.x == 0) s_base = total ? atomicAdd(&result[0], (unsigned long long)total) : 0ull;
        __syncthreads();
        uint64_t pos = s_base + before;   // (group-uniform) this group's first record
        // write: a group writes each record as whole 64-B runs, 16 B per lane, the mask applied in registers
#pragma unroll
        for (int k = 0; k < kExtractK; ++k) {
            const uint64_t b = b0 + (uint64_t)k * kCensusBktsPerBlock;
            const uint64_t s0 = u64_of(v[k].x, v[k].y), s1 = u64_of(v[k].z, v[k].w);
            uint32_t m8 = (uint32_t)(qm >> (8 * k)) & 0xFFu;
            while (m8) {   // (group-uniform)
                const int j = __ffs(m8) - 1;
                m8 &= m8 - 1;
                const uint64_t off = slot_off_raw(group_slot_word(s0, s1, j));
                const uint4 *ent = off_is_inline<IL>(off)
                                       ? reinterpret_cast<const uint4 *>(line + b * kLineBytes + kLineEntryOff)
                                       : reinterpret_cast<const uint4 *>(log + (off_of<IL>(off) & log_mask));
                if (pos < record_cap) {
                    const uint4 c = ent[q];
                    const uint64_t wa = u64_of(c.x, c.y) & mask_a, wb = u64_of(c.z, c.w) & mask_b;
                    uint4 *dst = records + pos * (4ull * chunks);
                    dst[q] = make_uint4((uint32_t)wa, (uint32_t)(wa >> 32), (uint32_t)wb, (uint32_t)(wb >> 32));
                    if (BIG)
                        for (uint32_t kk = 1; kk < chunks; ++kk) dst[4 * kk + q] = ent[4 * kk + q];
                }
                ++pos;
            }
        }
    }
    block_reduce(n_scanned, result + 1);
}

// One record per group of four lanes, one pass: the lanes load the record's first 64 B and look its key up as
// the reference does (first in-use tag match, window check, 8-byte key compare; IL: in the bucket's line, whose
// second half is the inline key's entry -- its log copy is neither read nor written). Lane 1 holds the entry's
// meta and the record's and decides: hermes_exec_inv of an INV with the record's timestamp, value and sender =
// ts cid, RMW flag 0 (on a table without RMWs), then hermes_exec_val when the record is VALID. The lanes write
// back only the 16-B chunks of bytes 16..63 that changed; the lock byte, ack_bv, op buffer index and last-local-
// write timestamp go back as they were read. A 320-B entry's other 256 value bytes move 64 consecutive bytes
// per group and instruction. No key occurs twice, so no two groups share an entry.
// FLAGS (the upsert's first step, hermeskv.h "Upsert"): also missed_flag[i] = 1 when record i was missed, else 0 --
// a template parameter, so that the install's own instances are the code they were.
enum : uint32_t { kMissed = 0, kOlder = 1, kEqual = 2, kRaised = 3 };

// Lane 1's decision: ln = the entry's bytes 16..31, r = the record's. hermes_exec_inv of the record's INV, then
// hermes_exec_val when the record is VALID, on a table without RMWs; nl = the bytes afterwards. The upsert's log
// writer applies the same to the image it inserts.
__device__ __forceinline__ uint32_t install_decide(const uint4 &ln, const uint4 &r, uint32_t kvs_value, uint4 &nl)
{
    uint32_t d;
    uint32_t w4 = ln.x, w5 = ln.y, ver = ln.z;
    const uint32_t r_state = (r.x >> 16) & 0xFFu, r_cid = r.y >> 24, r_ver = r.z;
    const uint64_t its = ((uint64_t)r_ver << 8) | r_cid, cur = ((uint64_t)ver << 8) | (w5 >> 24);
    if (its > cur) {   // hermes_exec_inv, the newer INV
        d = kRaised;
        const uint32_t st = (w4 >> 16) & 0xFFu;
        const uint32_t ns = st == kValid ? kInvalid : (st == kWrite || st == kReplay) ? kInvalidWrite : st;
        w4 = (w4 & 0xFF0000FFu) | ((kvs_value & 0xFFu) << 8) | (ns << 16);        // val_len, state
        w5 = (w5 & 0x00FFFF00u) | ((r_cid & 0x7Fu) << 1) | (r_cid << 24);         // RMW flag 0, last writer, ts cid
        ver = r_ver;
    } else if (its == cur) {
        d = kEqual;
        w5 = (w5 & ~0xFEu) | ((r_cid & 0x7Fu) << 1);                              // last writer
    } else {
        d = kOlder;
    }
    if (d >= kEqual && r_state == kValid) w4 = (w4 & 0xFF00FFFFu) | ((uint32_t)kValid << 16);   // hermes_exec_val
    nl.x = w4;
    nl.y = w5;
    nl.z = ver;
    return d;
}

template <bool IL, bool BIG, bool FLAGS>
__global__ __launch_bounds__(kCensusBlock) void k_table_install(const uint8_t *__restrict__ index, uint8_t *log,
                                                                uint8_t *line, const uint4 *__restrict__ records,
                                                                uint64_t n, uint64_t bkt_mask, uint64_t log_mask,
                                                                uint64_t log_head, uint64_t log_cap,
                                                                uint32_t kvs_value, uint32_t chunks,
                                                                unsigned long long *result,
                                                                uint8_t *__restrict__ missed_flag)
{
    Geometry g{};   // (the fields the probe reads)
    g.bkt_mask = bkt_mask, g.log_mask = log_mask, g.log_head = log_head, g.log_cap = log_cap;
    const uint64_t E4 = BIG ? 4ull * chunks : 4ull;   // 16-B chunks of a record
    const int q = threadIdx.x & 3, gbase = (threadIdx.x & 63) & ~3;
    uint32_t cnt[4] = {0, 0, 0, 0};   // raised, equal, older, missed: lane 1 of a group counts for it
    // a persistent grid striding over the records: the counts stay in registers until the block's end (one block
    // per 64 records, each ending in its own atomics on the four result words, measured 19 ms for 100M records)
    for (uint64_t i0 = (uint64_t)blockIdx.x * kCensusBktsPerBlock; i0 < n;
         i0 += (uint64_t)gridDim.x * kCensusBktsPerBlock) {   // (block-uniform)
        const uint64_t i = i0 + (threadIdx.x >> 2);
        const bool live = i < n;   // (the four lanes of a group share i)
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (live) r = records[i * E4 + q];
        const uint64_t key = __shfl(u64_of(r.z, r.w), 0, 4);
        const uint64_t bkt = bucket_of(g, key);
        uint4 v = make_uint4(0u, 0u, 0u, 0u), ev = v;
        if (live) {
            const uint4 *src = IL ? line_words(line, bkt) : bucket_words(index, bkt);
            v = src[q];
            if (IL) ev = src[4 + q];
        }
        bool ok, il;
        uint64_t phys;
        group_probe<IL>(u64_of(v.x, v.y), u64_of(v.z, v.w), key, live, gbase, g, ok, phys, il);
        // where the entry's bytes live: the line's second half for the bucket's inline key, else the log
        uint4 *home = reinterpret_cast<uint4 *>(il ? line_entry_of_bucket(line, bkt) : log + phys);
        uint4 ln = make_uint4(0u, 0u, 0u, 0u);
        if (ok) ln = il ? ev : home[q];
        const bool hit = ok && __shfl(u64_of(ln.z, ln.w), 0, 4) == key;
        uint32_t d = kMissed;
        uint4 nl = ln;
        if (q == 1 && hit) d = install_decide(ln, r, kvs_value, nl);   // ln: entry bytes 16..31; r: the record's
        d = __shfl(d, 1, 4);
        if (d == kRaised) {   // the value: bytes 33..63 here (byte 32 is the entry's own), the rest below
            if (q == 2) nl = make_uint4((ln.x & 0xFFu) | (r.x & ~0xFFu), r.y, r.z, r.w);
            if (q == 3) nl = r;
        }
        if (hit && q > 0 && !(nl.x == ln.x && nl.y == ln.y && nl.z == ln.z && nl.w == ln.w)) home[q] = nl;
        if (BIG && d == kRaised) {   // (the value's 64-B runs after the first, chunks - 1 of them, four at a time with
                                     // their loads before their stores: 320-B entries have exactly four, other sizes
                                     // end with a group of one to three)
            for (uint32_t k0 = 1; k0 < chunks; k0 += 4) {
                uint4 t[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    t[k] = k0 + k < chunks ? records[i * E4 + 4 * (k0 + k) + q] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (k0 + k < chunks) home[4 * (k0 + k) + q] = t[k];
            }
        }
        const bool mine = q == 1 && live;
        if (FLAGS) {
            // a wave's 16 records are 16 consecutive flag bytes: one 16-B store by its first lane instead of 16
            // byte stores (measured level with them). The store may run up to 63 bytes past n, inside
            // the flags' allocation (the caller rounds it up), with zero bytes.
            const unsigned long long bm = __ballot(mine && d == kMissed);   // bit 4g + 1: the wave's g-th record
            if ((threadIdx.x & 63) == 0) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t nib = (uint32_t)(bm >> (16 * k + 1));   // bits 0, 4, 8, 12: four records
                    w[k] = (nib & 1u) | ((nib >> 4 & 1u) << 8) | ((nib >> 8 & 1u) << 16) | ((nib >> 12 & 1u) << 24);
                }
                uint8_t *dst = missed_flag + i0 + (threadIdx.x >> 6) * 16;   // (i0 is a multiple of 64)
                *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        cnt[0] += mine && d == kRaised;
        cnt[1] += mine && d == kEqual;
        cnt[2] += mine && d == kOlder;
        cnt[3] += mine && d == kMissed;
    }
    block_reduce(cnt, result);
}

int launch_table_extract(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                         uint64_t bkt_lo, uint64_t bkt_hi, uint64_t min_ts, uint8_t *records, uint64_t record_cap,
                         unsigned long long *result, const uint8_t *part_sel, uint32_t part_bits, int device,
                         hipStream_t s)
{
    if (g.entry_size % 64 || (line && g.entry_size != 64) || bkt_lo > bkt_hi) return -1;
    if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) return -2;
    if (bkt_lo == bkt_hi) return 0;
    const uint32_t chunks = g.entry_size / 64;
    const uint64_t part_mask_of = (1ull << part_bits) - 1;
    with_instance(line != nullptr, chunks > 1, [&](auto il, auto big) {
        const auto launch = [&](auto k) {
            const dim3 grid = persistent_grid((const void *)k, bkt_hi - bkt_lo, kExtractBktsPerStep, device, 8);
            hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, index, log, line, bkt_lo, bkt_hi, g.log_mask, g.log_head, g.log_cap, chunks, min_ts,
                               reinterpret_cast<uint4 *>(records), record_cap, result, part_sel, part_mask_of);
        };
        if (part_sel) launch(k_table_extract<decltype(il)::value, decltype(big)::value, true>);
        else launch(k_table_extract<decltype(il)::value, decltype(big)::value, false>);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_table_install(const Geometry &g, const uint8_t *index, uint8_t *log, uint8_t *line, const uint8_t *records,
                         uint64_t n, unsigned long long *result, hipStream_t s, uint8_t *missed_flag)
{
    const uint32_t chunks = g.entry_size / 64;
    const bool big = chunks > 1;
    if (g.entry_size % 64 || (line && big) || g.rmw_enabled) return -1;
    if (hipMemsetAsync(result, 0, 4 * sizeof(unsigned long long), s) != hipSuccess) return -2;
    if (!n) return 0;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) device = -1;   // (no device: the grid falls back to 256 CUs)
    // 8 blocks per CU, what the CUs hold at once at the instances' 8 waves per SIMD: no occupancy query
    const dim3 grid = persistent_grid(nullptr, n, kCensusBktsPerBlock, device, 8);
    with_instance(line != nullptr, big, [&](auto il, auto bg) {
        const auto launch = [&](auto k) {
            hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, index, log, line,
                               reinterpret_cast<const uint4 *>(records), n, g.bkt_mask, g.log_mask, g.log_head,
                               g.log_cap, g.kvs_value, chunks, result, missed_flag);
        };
        if (missed_flag) launch(k_table_install<decltype(il)::value, decltype(bg)::value, true>);
        else launch(k_table_install<decltype(il)::value, decltype(bg)::value, false>);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------ key-level delta repair: summaries, need, fetch
// hermeskv.h "Key-level delta repair". Three read-only passes: the extract's pass that leaves 16 B per key instead
// of a record, the install's lookup that only classes, and the install's lookup that copies the entry out.
//
// k_table_summaries is k_table_extract in its count and reserve parts -- the same loads, the same liveness, mask
// and min_ts rules, one returning atomic per block and step -- written out again so that the extract's instances
// stay the code they are. Its write part differs: a summary needs an entry's bytes 8..31 only, so instead of four
// lanes moving one record together, each lane of the group takes one of the bucket's records (the q-th, then the
// q+4-th), loads the entry's first 32 B -- one sector, whatever the entry size, which is why there is no BIG
// instance -- and stores one whole 16-B summary. (Each lane writing the summaries of the two slots whose words it
// already holds needs no shuffle, but its work follows the slots -- which fill from slot 7 down, so lane 3 does
// most of it -- and its IL instance takes 133 VGPRs: measured slower at every selection)
template <bool IL, bool MASKED>
__global__ __launch_bounds__(kCensusBlock) void k_table_summaries(const uint8_t *__restrict__ index,
                                                                  const uint8_t *__restrict__ log,
                                                                  const uint8_t *__restrict__ line, uint64_t bkt_lo,
                                                                  uint64_t bkt_hi, uint64_t log_mask, uint64_t log_head,
                                                                  uint64_t log_cap, uint64_t min_ts,
                                                                  uint4 *__restrict__ summaries, uint64_t cap,
                                                                  unsigned long long *result,
                                                                  const uint8_t *__restrict__ part_sel,
                                                                  uint64_t part_mask_of)
{
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63, gbase = lane & ~3, wave = threadIdx.x >> 6;
    const uint64_t tiles = (bkt_hi - bkt_lo + kExtractBktsPerStep - 1) / kExtractBktsPerStep;
    __shared__ unsigned long long s_wtot[kCensusBlock / 64], s_base;
    uint32_t n_scanned[1] = {0};
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform)
        const uint64_t b0 = bkt_lo + tile * kExtractBktsPerStep + (threadIdx.x >> 2);   // (the four lanes of a group share it)
        // count: as k_table_extract (bit 8k + j: slot j of bucket k leaves as a summary)
        uint4 v[kExtractK];
#pragma unroll
        for (int k = 0; k < kExtractK; ++k) {
            const uint64_t b = b0 + (uint64_t)k * kCensusBktsPerBlock;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (b < bkt_hi && (!MASKED || part_sel[b & part_mask_of]))
                v[k] = (IL ? line_words(line, b) : bucket_words(index, b))[q];
        }
        uint64_t qm = 0;
#pragma unroll
        for (int k = 0; k < kExtractK; ++k) {
            const uint64_t b = b0 + (uint64_t)k * kCensusBktsPerBlock;
            const uint64_t s0 = u64_of(v[k].x, v[k].y), s1 = u64_of(v[k].z, v[k].w);
            uint32_t o = group_slots(slot_in_use(s0) && in_log_window(log_head, log_cap, off_of<IL>(slot_off_raw(s0))),
                                     slot_in_use(s1) && in_log_window(log_head, log_cap, off_of<IL>(slot_off_raw(s1))), gbase);
            if (q == 0) n_scanned[0] += __popc(o);
            if (min_ts) {   // (uniform)
                uint32_t left = o;
                while (left) {   // (group-uniform)
                    const int j = __ffs(left) - 1;
                    left &= left - 1;
                    const uint64_t off = slot_off_raw(group_slot_word(s0, s1, j));
                    const uint4 m = off_is_inline<IL>(off)
                                        ? reinterpret_cast<const uint4 *>(line + b * kLineBytes + kLineEntryOff)[1]
                                        : reinterpret_cast<const uint4 *>(log + (off_of<IL>(off) & log_mask))[1];
                    if ((((uint64_t)m.z << 8) | (m.y >> 24)) < min_ts) o &= ~(1u << j);
                }
            }
            qm |= (uint64_t)o << (8 * k);
        }
        // reserve: as k_table_extract, one returning atomic on the counter per block and step
        const uint32_t cnt = (uint32_t)__popcll(qm);
        uint32_t x = q == 0 ? cnt : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const uint32_t excl = (uint32_t)__shfl(x, 0, 4) - cnt;
        const uint32_t wtot = (uint32_t)__shfl(x, 63);
        if (lane == 0) s_wtot[wave] = wtot;
        __syncthreads();
        uint64_t before = excl, total = 0;
#pragma unroll
        for (int w = 0; w < kCensusBlock / 64; ++w) {
            const uint64_t t = s_wtot[w];
            if (w < wave) before += t;
            total += t;
        }
        if (threadIdx.x == 0) s_base = total ? atomicAdd(&result[0], (unsigned long long)total) : 0ull;
        __syncthreads();
        uint64_t pos = s_base + before;   // (group-uniform) this group's first summary
        // write: lane q takes the bucket's q-th record, then its q+4-th
#pragma unroll
        for (int k = 0; k < kExtractK; ++k) {
            const uint64_t b = b0 + (uint64_t)k * kCensusBktsPerBlock;
            const uint64_t s0 = u64_of(v[k].x, v[k].y), s1 = u64_of(v[k].z, v[k].w);
            const uint32_t m8 = (uint32_t)(qm >> (8 * k)) & 0xFFu, nk = __popc(m8);
            for (uint32_t r = 0; r < nk; r += 4) {   // (group-uniform)
                uint32_t m = m8;
#pragma unroll
                for (uint32_t t = 0; t < 7; ++t)
                    if (t < r + q) m &= m - 1;   // drop the records before mine
                const int j = m ? __ffs(m) - 1 : 0;
                // slot j's word lives in lane j >> 1 (j differs per lane here, so both of that lane's words travel)
                const uint64_t w0 = __shfl(s0, j >> 1, 4), w1 = __shfl(s1, j >> 1, 4);
                const uint64_t off = slot_off_raw((j & 1) ? w1 : w0);
                if (m && pos + r + q < cap) {
                    const uint4 *ent = off_is_inline<IL>(off)
                                           ? reinterpret_cast<const uint4 *>(line + b * kLineBytes + kLineEntryOff)
                                           : reinterpret_cast<const uint4 *>(log + (off_of<IL>(off) & log_mask));
                    const uint4 e0 = ent[0], e1 = ent[1];   // bytes 8..15: the key; 18 state, 23 ts cid, 24..27 ts version
                    summaries[pos + r + q] = make_uint4(e0.z, e0.w, e1.z, (e1.y >> 24) | (((e1.x >> 16) & 0xFFu) << 8));
                }
            }
            pos += nk;
        }
    }
    block_reduce(n_scanned, result + 1);
}

// word indices of hkv_need_result
enum : uint32_t { kNdMissed = 0, kNdNewer = 1, kNdValidate = 2, kNdSame = 3, kNdStateOnly = 4, kNdOlder = 5, kNdNeeded = 6 };

// One summary per group of four lanes: the install's lookup (group_probe, then the 8-byte key compare on the
// entry's first 16 B), and lane 1, which holds the entry's bytes 16..31, classes the summary against them. Only
// the entry's first 32 B are read, so one instance serves every entry size. The six counts stay in registers
// until the block's end; the needed keys are compacted with the extract's reservation -- a ballot per wave, the
// waves' totals through LDS, ONE returning atomic on result[kNdNeeded] per block and step.
template <bool IL>
__global__ __launch_bounds__(kCensusBlock) void k_table_need(const uint8_t *__restrict__ index,
                                                             const uint8_t *__restrict__ log,
                                                             const uint8_t *__restrict__ line,
                                                             const uint4 *__restrict__ summaries, uint64_t n,
                                                             uint64_t bkt_mask, uint64_t log_mask, uint64_t log_head,
                                                             uint64_t log_cap, unsigned long long *__restrict__ need_keys,
                                                             uint64_t need_cap, unsigned long long *result)
{
    Geometry g{};   // (the fields the probe reads)
    g.bkt_mask = bkt_mask, g.log_mask = log_mask, g.log_head = log_head, g.log_cap = log_cap;
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63, gbase = lane & ~3, wave = threadIdx.x >> 6;
    __shared__ unsigned long long s_wtot[kCensusBlock / 64], s_base;
    uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};   // lane 1 of a group counts for it
    for (uint64_t i0 = (uint64_t)blockIdx.x * kCensusBktsPerBlock; i0 < n;
         i0 += (uint64_t)gridDim.x * kCensusBktsPerBlock) {   // (block-uniform)
        const uint64_t i = i0 + (threadIdx.x >> 2);
        const bool live = i < n;   // (the four lanes of a group share i)
        uint4 sm = make_uint4(0u, 0u, 0u, 0u);
        if (live) sm = summaries[i];
        const uint64_t key = u64_of(sm.x, sm.y);
        const uint64_t bkt = bucket_of(g, key);
        uint4 v = make_uint4(0u, 0u, 0u, 0u), ev = v;
        if (live) {
            const uint4 *src = IL ? line_words(line, bkt) : bucket_words(index, bkt);
            v = src[q];
            if (IL && q < 2) ev = src[4 + q];
        }
        bool ok, il;
        uint64_t phys;
        group_probe<IL>(u64_of(v.x, v.y), u64_of(v.z, v.w), key, live, gbase, g, ok, phys, il);
        const uint4 *home = reinterpret_cast<const uint4 *>(il ? line_entry_of_bucket(line, bkt) : log + phys);
        uint4 ln = make_uint4(0u, 0u, 0u, 0u);
        if (ok && q < 2) ln = il ? ev : home[q];   // lane 0: the key; lane 1: bytes 16..31
        const bool hit = ok && __shfl(u64_of(ln.z, ln.w), 0, 4) == key;
        uint32_t cls = kNdMissed;
        if (hit) {   // (lane 1's is the group's)
            const uint32_t st = (ln.x >> 16) & 0xFFu, s_st = (sm.w >> 8) & 0xFFu;
            const uint64_t cur = ((uint64_t)ln.z << 8) | (ln.y >> 24), its = ((uint64_t)sm.z << 8) | (sm.w & 0xFFu);
            cls = its > cur ? kNdNewer : its < cur ? kNdOlder : s_st == st ? kNdSame : s_st == kValid ? kNdValidate : kNdStateOnly;
        }
        const bool mine = q == 1 && live, need = mine && cls <= kNdValidate;
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k) cnt[k] += mine && cls == k;
        const unsigned long long bm = __ballot(need);
        if (lane == 0) s_wtot[wave] = (unsigned long long)__popcll(bm);
        __syncthreads();
        uint64_t before = (uint64_t)__popcll(bm & ((1ull << lane) - 1)), total = 0;
#pragma unroll
        for (int w = 0; w < kCensusBlock / 64; ++w) {
            const uint64_t t = s_wtot[w];
            if (w < wave) before += t;
            total += t;
        }
        if (threadIdx.x == 0) s_base = total ? atomicAdd(&result[kNdNeeded], (unsigned long long)total) : 0ull;
        __syncthreads();
        if (need && s_base + before < need_cap) need_keys[s_base + before] = key;
    }
    block_reduce(cnt, result);
}

// One key per group of four lanes, record i to records[i]: the install's lookup, then the entry leaves as the
// extract writes a record -- whole 64-B runs, 16 B per lane, the digest's mask applied in registers, a 320-B
// entry's further runs 64 consecutive bytes per group and instruction, four at a time with their loads before
// their stores. A key the table does not hold leaves a zero record with its key in bytes 8..15.
template <bool IL, bool BIG>
__global__ __launch_bounds__(kCensusBlock) void k_table_fetch(const uint8_t *__restrict__ index,
                                                              const uint8_t *__restrict__ log,
                                                              const uint8_t *__restrict__ line,
                                                              const unsigned long long *__restrict__ keys, uint64_t n,
                                                              uint64_t bkt_mask, uint64_t log_mask, uint64_t log_head,
                                                              uint64_t log_cap, uint32_t chunks,
                                                              uint4 *__restrict__ records, unsigned long long *result)
{
    Geometry g{};   // (the fields the probe reads)
    g.bkt_mask = bkt_mask, g.log_mask = log_mask, g.log_head = log_head, g.log_cap = log_cap;
    const uint64_t E4 = BIG ? 4ull * chunks : 4ull;   // 16-B chunks of a record
    const int q = threadIdx.x & 3, gbase = (threadIdx.x & 63) & ~3;
    const uint64_t mask_a = digest_mask_a(q), mask_b = digest_mask_b(q);
    uint32_t cnt[2] = {0, 0};   // found, absent: lane 1 of a group counts for it
    for (uint64_t i0 = (uint64_t)blockIdx.x * kCensusBktsPerBlock; i0 < n;
         i0 += (uint64_t)gridDim.x * kCensusBktsPerBlock) {   // (block-uniform)
        const uint64_t i = i0 + (threadIdx.x >> 2);
        const bool live = i < n;   // (the four lanes of a group share i)
        const uint64_t key = live ? keys[i] : 0ull;
        const uint64_t bkt = bucket_of(g, key);
        uint4 v = make_uint4(0u, 0u, 0u, 0u), ev = v;
        if (live) {
            const uint4 *src = IL ? line_words(line, bkt) : bucket_words(index, bkt);
            v = src[q];
            if (IL) ev = src[4 + q];
        }
        bool ok, il;
        uint64_t phys;
        group_probe<IL>(u64_of(v.x, v.y), u64_of(v.z, v.w), key, live, gbase, g, ok, phys, il);
        const uint4 *home = reinterpret_cast<const uint4 *>(il ? line_entry_of_bucket(line, bkt) : log + phys);
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        if (ok) c = il ? ev : home[q];
        const bool hit = ok && __shfl(u64_of(c.z, c.w), 0, 4) == key;
        const uint64_t wa = hit ? u64_of(c.x, c.y) & mask_a : 0ull;
        const uint64_t wb = hit ? u64_of(c.z, c.w) & mask_b : q == 0 ? key : 0ull;
        uint4 *dst = records + i * E4;
        if (live) dst[q] = make_uint4((uint32_t)wa, (uint32_t)(wa >> 32), (uint32_t)wb, (uint32_t)(wb >> 32));
        if (BIG && live) {
            for (uint32_t k0 = 1; k0 < chunks; k0 += 4) {
                uint4 t[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    t[k] = hit && k0 + k < chunks ? home[4 * (k0 + k) + q] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (k0 + k < chunks) dst[4 * (k0 + k) + q] = t[k];
            }
        }
        cnt[0] += q == 1 && live && hit;
        cnt[1] += q == 1 && live && !hit;
    }
    block_reduce(cnt, result);
}

int launch_table_summaries(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                           uint64_t bkt_lo, uint64_t bkt_hi, uint64_t min_ts, uint8_t *summaries, uint64_t cap,
                           unsigned long long *result, const uint8_t *part_sel, uint32_t part_bits, int device,
                           hipStream_t s)
{
    if (g.entry_size % 64 || (line && g.entry_size != 64) || bkt_lo > bkt_hi) return -1;
    if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) return -2;
    if (bkt_lo == bkt_hi) return 0;
    const uint64_t part_mask_of = (1ull << part_bits) - 1;
    const auto launch = [&](auto k) {
        const dim3 grid = persistent_grid((const void *)k, bkt_hi - bkt_lo, kExtractBktsPerStep, device, 8);
        hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, index, log, line, bkt_lo, bkt_hi, g.log_mask, g.log_head, g.log_cap, min_ts,
                           reinterpret_cast<uint4 *>(summaries), cap, result, part_sel, part_mask_of);
    };
    if (line) part_sel ? launch(k_table_summaries<true, true>) : launch(k_table_summaries<true, false>);
    else part_sel ? launch(k_table_summaries<false, true>) : launch(k_table_summaries<false, false>);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_table_need(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                      const uint8_t *summaries, uint64_t n, unsigned long long *need_keys, uint64_t need_cap,
                      unsigned long long *result, int device, hipStream_t s)
{
    if (g.entry_size % 64 || (line && g.entry_size != 64)) return -1;
    if (hipMemsetAsync(result, 0, 8 * sizeof(unsigned long long), s) != hipSuccess) return -2;
    if (!n) return 0;
    const dim3 grid = persistent_grid(nullptr, n, kCensusBktsPerBlock, device, 8);
    const auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, index, log, line, reinterpret_cast<const uint4 *>(summaries), n, g.bkt_mask, g.log_mask,
                           g.log_head, g.log_cap, need_keys, need_cap, result);
    };
    line ? launch(k_table_need<true>) : launch(k_table_need<false>);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_table_fetch(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                       const unsigned long long *keys, uint64_t n, uint8_t *records, unsigned long long *result,
                       int device, hipStream_t s)
{
    const uint32_t chunks = g.entry_size / 64;
    if (g.entry_size % 64 || (line && chunks > 1)) return -1;
    if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) return -2;
    if (!n) return 0;
    const dim3 grid = persistent_grid(nullptr, n, kCensusBktsPerBlock, device, 8);
    with_instance(line != nullptr, chunks > 1, [&](auto il, auto big) {
        hipLaunchKernelGGL((k_table_fetch<decltype(il)::value, decltype(big)::value>), grid, dim3(kCensusBlock), 0, s, index, log, line, keys, n,
                           g.bkt_mask, g.log_mask, g.log_head, g.log_cap, chunks, reinterpret_cast<uint4 *>(records), result);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------ upsert: the inserts
// hermeskv.h "Upsert", step 2, after the install with FLAGS has marked the missed records and the host has read
// their number m. Rank: an exclusive scan of the flags gives each missed record its place among them in record
// order -- its log rank, which plan_off turns into the offset mica_insert_one would hand out (an atomic append
// would make the log order a matter of scheduling). Pairs: rank r's bucket and r itself, with key[r] and the
// record's index beside them; the stable sort by bucket and the populate's k_pop_buckets then replay each bucket's
// inserts in rank order, which is record order. Log: one group of four lanes per rank reads its record once, forms
// the final entry in registers and writes it as whole 64-byte runs, 16 B per lane.
namespace {
struct FlagToRank {
    __device__ uint32_t operator()(uint8_t f) const { return f ? 1u : 0u; }
};
}  // namespace

size_t scan_temp_bytes(uint64_t n)
{
    size_t bytes = 0;
    rocprim::exclusive_scan(nullptr, bytes, rocprim::make_transform_iterator((const uint8_t *)nullptr, FlagToRank{}),
                            (uint32_t *)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>());
    return bytes;
}

__global__ __launch_bounds__(kCensusBlock) void k_ups_pairs(const uint8_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ ranks,
                                                            const uint8_t *__restrict__ records, uint64_t n,
                                                            uint32_t entry_size, uint64_t bkt_mask,
                                                            uint32_t *__restrict__ bkt_keys, uint32_t *__restrict__ pos,
                                                            uint64_t *__restrict__ key_of,
                                                            uint32_t *__restrict__ rec_of)
{
    const uint64_t step = (uint64_t)gridDim.x * kCensusBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCensusBlock + threadIdx.x; i < n; i += step) {
        if (!flags[i]) continue;
        const uint32_t r = ranks[i];   // (below m, the flags' total, which sized the arrays)
        const uint64_t key = *reinterpret_cast<const uint64_t *>(records + i * entry_size + 8);
        bkt_keys[r] = (uint32_t)((key & 0xFFFFFFFFu) & bkt_mask);   // mica_insert_one: 32-bit bkt field
        pos[r] = r;
        key_of[r] = key;
        rec_of[r] = (uint32_t)i;
    }
}

// The entry an inserted record leaves (hermeskv.h "Upsert", step 2): the populate image (k_pop_log) with bytes
// 0..7 zero, the record's key and value, then the record's INV and VAL applied to it as the install applies them.
template <bool BIG>
__global__ __launch_bounds__(kCensusBlock) void k_ups_log(const uint4 *__restrict__ records,
                                                          const uint32_t *__restrict__ rec_of, uint8_t *log,
                                                          uint64_t p_begin, uint64_t p_end, LogPlan L,
                                                          uint64_t log_mask, uint32_t kvs_value, uint32_t val_len_byte, uint32_t chunks)
{
    const uint64_t E4 = BIG ? 4ull * chunks : 4ull;   // 16-B chunks of a record
    const int q = threadIdx.x & 3;
    for (uint64_t p0 = p_begin + (uint64_t)blockIdx.x * kCensusBktsPerBlock; p0 < p_end;
         p0 += (uint64_t)gridDim.x * kCensusBktsPerBlock) {   // (block-uniform)
        const uint64_t p = p0 + (threadIdx.x >> 2);
        if (p >= p_end) continue;   // (the four lanes of a group share p; nothing below crosses lanes)
        const uint64_t i = rec_of[p];
        const uint4 r = records[i * E4 + q];
        uint4 img = r;   // q == 3: value bytes
        if (q == 0) img = make_uint4(0u, 0u, r.z, r.w);   // no key_first; the key
        if (q == 1) {
            // bytes 16..23: opcode PUT, val_len, state VALID, ack_bv 0, lwid 127, obi 255, lock 0, cid 255; 24..31: 0
            const uint32_t w4 = (uint32_t)kOpPut | (val_len_byte << 8) | ((uint32_t)kValid << 16);
            const uint32_t w5 = (uint32_t)(kLwidEmpty << 1) | ((uint32_t)kObiEmpty << 8) | ((uint32_t)kCidEmpty << 24);
            const uint4 ln = make_uint4(w4, w5, 0u, 0u);
            img = ln;
            (void)install_decide(ln, r, kvs_value, img);
        }
        if (q == 2) img.x = r.x & ~0xFFu;   // byte 32 is the entry's own (last-local-write version), the value from 33
        uint4 *dst = reinterpret_cast<uint4 *>(log + (plan_off(L, p) & log_mask));
        dst[q] = img;
        if (BIG)
            for (uint32_t k = 1; k < chunks; ++k) dst[4 * k + q] = records[i * E4 + 4 * k + q];
    }
}

int launch_upsert_inserts(const UpsertLaunch &u, hipStream_t s)
{
    const Geometry &g = u.g;
    const uint32_t chunks = g.entry_size / 64;
    if (g.entry_size % 64 || !u.m || u.m > u.n || u.n > 0x7FFFFFFFull || (u.h0 & 15)) return -1;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) device = -1;
    const auto mark = [&](int k) {
        if (u.phase_events) (void)hipEventRecord(u.phase_events[k], s);
    };
    size_t scan_bytes = u.scan_tmp_bytes;
    if (rocprim::exclusive_scan(u.scan_tmp, scan_bytes,
                                rocprim::make_transform_iterator(u.flags, FlagToRank{}), u.ranks, 0u, (size_t)u.n,
                                rocprim::plus<uint32_t>(), s) != hipSuccess)
        return -2;
    hipLaunchKernelGGL(k_ups_pairs, persistent_grid(nullptr, u.n, kCensusBlock, device, 8), dim3(kCensusBlock), 0, s,
                       u.flags, u.ranks, u.records, u.n, g.entry_size, g.bkt_mask, u.keys_a, u.vals_a, u.key_of,
                       u.rec_of);
    if (hipGetLastError() != hipSuccess) return -3;
    mark(0);
    if (sort_pairs(u.sort_tmp, u.sort_tmp_bytes, u.keys_a, u.keys_b, u.vals_a, u.vals_b, (int64_t)u.m, u.key_bits, s))
        return -4;
    mark(1);
    LogPlan L{u.h0, u.k, u.hw, g.entry_size};
    hipLaunchKernelGGL(k_pop_buckets<true>, dim3((unsigned)((u.m + 255) / 256)), dim3(256), 0, s, u.keys_b, u.vals_b,
                       u.key_of, u.index, (int64_t)u.m, L, u.evictions, u.counts);
    if (hipGetLastError() != hipSuccess) return -5;
    mark(2);
    // as launch_populate: no launch overlaps itself across the single wrap or across one lap of the log, and the
    // launches run in rank order, so a later insert overwrites an earlier one where the reference's would
    uint64_t chunk = g.log_cap / g.entry_size;
    if (chunk < 1) chunk = 1;
    const uint64_t wrap_at = u.k < u.m ? u.k : u.m;
    const uint64_t runs[2][2] = {{0, wrap_at}, {wrap_at, u.m}};
    for (const auto &r : runs) {
        for (uint64_t b = r[0]; b < r[1]; b += chunk) {
            const uint64_t e = b + chunk < r[1] ? b + chunk : r[1];
            const dim3 grid = persistent_grid(nullptr, e - b, kCensusBktsPerBlock, device, 8);
            const auto recs = reinterpret_cast<const uint4 *>(u.records);
            const auto launch = [&](auto k) {
                hipLaunchKernelGGL(k, grid, dim3(kCensusBlock), 0, s, recs, u.rec_of, u.log, b, e, L, g.log_mask,
                                   g.kvs_value, (uint32_t)u.val_len_byte, chunks);
            };
            if (chunks > 1) launch(k_ups_log<true>);
            else launch(k_ups_log<false>);
            if (hipGetLastError() != hipSuccess) return -6;
        }
    }
    mark(3);
    return 0;
}

}  // namespace hkv
