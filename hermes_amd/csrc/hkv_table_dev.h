// hkv_table_dev.h -- the one statement of how device code reads the table (internal, device only): a slot's
// fields, a key's bucket and tag, the log window, the inline residency's line, and the reference's
// lookup (hermesKV.c:952-993: first in-use tag match in slot order, window check; the 8-byte key compare stays
// with the callers, who read the entry differently). Functions and constants only: no kernels, no state.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hkv_internal.h"

namespace hkv {

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// ---- a slot: bit 0 in use, bits 1..23 the tag, bits 24..63 the log offset (bit 39 of it: kInlineOffBit)
__device__ __forceinline__ bool slot_in_use(uint64_t slot) { return slot & 1u; }
__device__ __forceinline__ uint32_t slot_tag(uint64_t slot) { return (uint32_t)(slot >> 1) & 0x7FFFFFu; }
__device__ __forceinline__ uint32_t key_tag(uint64_t key) { return (uint32_t)(key >> 48); }
__device__ __forceinline__ bool slot_matches(uint64_t slot, uint32_t tag) { return slot_in_use(slot) && slot_tag(slot) == tag; }
// the offset field as stored (a line's flagged slot carries kInlineOffBit), and the log offset it names
__device__ __forceinline__ uint64_t slot_off_raw(uint64_t slot) { return slot >> 24; }
template <bool IL>
__device__ __forceinline__ bool off_is_inline(uint64_t raw) { return IL && (raw & kInlineOffBit); }
template <bool IL>
__device__ __forceinline__ uint64_t off_of(uint64_t raw) { return IL ? raw & ~kInlineOffBit : raw; }

__device__ __forceinline__ uint64_t bucket_of(const Geometry &g, uint64_t key) { return (key & 0xFFFFFFFFFFFFULL) & g.bkt_mask; }
// the lookup's wrap test (hermesKV.c:969-970): the log has not overwritten the entry at off
__device__ __forceinline__ bool in_log_window(uint64_t log_head, uint64_t log_cap, uint64_t off) { return log_head - off < log_cap; }
__device__ __forceinline__ bool in_log_window(const Geometry &g, uint64_t off) { return in_log_window(g.log_head, g.log_cap, off); }

// ---- addressing: a 64-B bucket of the index; a 128-B line (the bucket, then its inline key's 64-B entry)
constexpr uint32_t kBucketBytes = 64u, kLineBytes = 128u, kLineEntryOff = 64u;
template <class B>
using Words = std::conditional_t<std::is_const<B>::value, const uint4, uint4>;
__device__ __forceinline__ const uint4 *bucket_words(const uint8_t *index, uint64_t b) { return reinterpret_cast<const uint4 *>(index + b * kBucketBytes); }
template <class B>
__device__ __forceinline__ Words<B> *line_words(B *line, uint64_t b) { return reinterpret_cast<Words<B> *>(line + b * kLineBytes); }
template <class B>
__device__ __forceinline__ B *line_entry_of_bucket(B *line, uint64_t b) { return line + b * kLineBytes + kLineEntryOff; }
template <class B>
__device__ __forceinline__ B *line_entry(B *line, const Geometry &g, uint64_t key) { return line_entry_of_bucket(line, bucket_of(g, key)); }

// ---- four lanes per bucket: lane q of the group at lanes gbase..gbase+3 holds slots 2q (s0) and 2q + 1 (s1)
// p0, p1: this lane's predicate on its two slots; bit j of the result: slot j's. Every lane of the wave calls it.
__device__ __forceinline__ uint32_t group_slots(bool p0, bool p1, int gbase)
{
    const uint32_t g0 = (uint32_t)(__ballot(p0) >> gbase) & 0xFu;
    const uint32_t g1 = (uint32_t)(__ballot(p1) >> gbase) & 0xFu;
    uint32_t o = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) o |= ((g0 >> l) & 1u) << (2 * l) | ((g1 >> l) & 1u) << (2 * l + 1);
    return o;
}
// slot j's word (or whatever the lanes pass of their two slots), to all four lanes
__device__ __forceinline__ uint64_t group_slot_word(uint64_t s0, uint64_t s1, int j) { return __shfl((j & 1) ? s1 : s0, j >> 1, 4); }

// The lookup on the bucket words the group has loaded (an idle group passes live = false): ok, phys = the hit's
// offset in the log, and (IL instances) il: the hit is the bucket's inline key, whose entry is the line's second half.
template <bool IL>
__device__ __forceinline__ void group_probe(uint64_t s0, uint64_t s1, uint64_t key, bool live, int gbase,
                                            const Geometry &g, bool &ok, uint64_t &phys, bool &il)
{
    const uint32_t tag = key_tag(key);
    const uint32_t o = group_slots(live && slot_matches(s0, tag), live && slot_matches(s1, tag), gbase);
    const int first = o ? __ffs(o) - 1 : 0;
    const uint64_t raw = group_slot_word(slot_off_raw(s0), slot_off_raw(s1), first), off = off_of<IL>(raw);
    ok = live && o && in_log_window(g, off);
    phys = off & g.log_mask;
    il = off_is_inline<IL>(raw) && ok;
}

// ---- the digest's masks on lane q's two words (2q, 2q + 1) of an entry's first 64 B: key; state and ts cid,
// ts version; the value from byte 33 on (hermeskv.h "Table census and digest"; a repair record is that image)
__device__ __forceinline__ uint64_t digest_mask_a(int q) { return q == 0 ? 0ull : q == 1 ? 0xFF00000000FF0000ull : q == 2 ? 0xFFFFFFFFFFFFFF00ull : ~0ull; }
__device__ __forceinline__ uint64_t digest_mask_b(int q) { return q == 1 ? 0x00000000FFFFFFFFull : ~0ull; }

}  // namespace hkv
