// hkv_batch.hip -- the HermesKV batch path on gfx950 (hermes_batch_ops_to_KVS, hermesKV.c:905-996).
//
// One launch applies n_batches batches of one type. Its result is defined as the reference
// applying them element by element in concatenation order. Nothing is sorted: elements stay in
// element order, and the elements of each key are resolved in rounds.
//
//   k_lookup    one element per 4 lanes, in element order: skip test (hermesKV.c:709-769),
//               bucket probe over the 64-B bucket (hermesKV.c:952-975), wrap test, 8-B key
//               compare (hermesKV.c:977-993; a miss writes ST_MISS into byte 9). A hit reads
//               the key's object meta S_0 from the same log line and offers itself as round
//               0's first candidate if would_mutate(elem, S_0) (hkv_exec.h).
//   round r     every key keeps F_r, the smallest element index among its candidates (one
//               atomicMin on the F word of the key's log line). Then
//                 k_resolve: an element before F_r (or of a key without a candidate) sees S_r in
//                   the sequential order and S_r does not change under it: it runs the
//                   reference's exec function on a private copy of S_r against the live entry,
//                   in parallel with everything else. F_r itself runs the exec function on a
//                   shadow image of the entry (S_r -> S_{r+1}), so the entry still holds S_r for
//                   every concurrent reader; later elements stay pending.
//                 k_cand (r+1): every pending element tests would_mutate against S_{r+1}, read
//                   from the shadow of round r's first candidate; k_commit copies each key's
//                   last shadow into its entry once, after the last round.
//   fallback    elements still pending after the last round (keys mutated in every round) are
//               gathered per key into workgroup-owned lists (key -> workgroup by its last first
//               candidate), sorted by element index in LDS, and finished in element order: runs
//               of up to 32 by one thread, longer runs by the whole workgroup with block-wide
//               first-candidate passes over chunks (k_fb_exec).
//
// Exactness rests on one property: would_mutate() is sound (false => the exec function leaves
// the meta unchanged). Every resolved element checks it: a private copy that did change raises
// bit 0 of *error_flags, which every parity test asserts is zero.
//
// Slots and F words are tagged with the launch (key word) and the round (F word), so no scratch
// is cleared between launches: a slot whose tag is older reads as empty, and a newer round's F
// value is numerically smaller than every older one, so atomicMin replaces stale words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hkv_batch_dev.h"   // BatchArgs, BatchPlan, the shared helpers; see its file map

namespace hkv {

// Rounds after round 0 per batch type: how often a hot key usually mutates in one launch beyond
// the first time. An ACK batch sets an ack bit and then completes; INVs carry at most a few
// distinct timestamps per key and launch. Keys that mutate more go to the fallback.
// None for VAL batches and for local batches without RMWs: their first mutation leaves the key in
// an absorbing state (absorbing_state), so k_resolve0 finishes every key.
__host__ __device__ constexpr int rounds_for(int type, bool rmw)
{
    return type == kVals || (type == kLocal && !rmw) ? 0 : 2;
}

// INV direct path (INV launches without RMWs, fewer than 2^23 elements). Without RMWs,
// hermes_exec_inv (hermesKV.c:489-588) on one key, element by element from S_0, comes to this:
// let M be the largest INV timestamp of the key's elements.
//   M > ts_0:  the first element with ts M (A) installs its value, RMW flag and M; the state moves
//              once (VALID -> INVALID, WRITE/REPLAY -> INVALID_WRITE, others stay), val_len :=
//              KVS_VALUE_SIZE; last_writer_id := sender of the last element with ts M (B).
//   M = ts_0:  last_writer_id := sender of the last element with ts ts_0 (B); nothing else.
//   M < ts_0:  nothing.
// Every element's opcode is INV_SUCCESS (an INV_ABORT / OUT_OF_GROUP input stays), except
// OUT_OF_GROUP for an element with ts = ts_0 in state WRITE, which holds until the first element
// with a larger ts (P). Per key (log line) three words:
//   X = max over raising elements of (ts << 24 | ~i) -> M and A (k_lookup);
//   F = round 0's word: P, offered by raising elements of keys in state WRITE (k_lookup);
//   Y = 1 + B when B != A (k_inv_resolve), or for keys without a raise.
// k_lookup finishes the elements below ts_0; k_inv_resolve writes the other opcodes, A keeps X in
// its own scratch slot (mem[A]) and the other elements with ts M flag A's slot pf[A] ("B is not
// A") and raise Y; in k_inv_commit A (or, without a raise, B) applies the key's meta and clears X
// and Y. Most keys of a launch have one element: it is A and B, never touches Y, and commits from
// its own slots without reading X again.
enum : uint8_t { kIvRaise = 1, kIvEq = 2, kIvWrite = 4, kIvCand = 8, kIvApply = 16 };
constexpr int64_t kInvDirectMax = 1 << 23;

// ACK direct path (ACK launches without RMWs). Without RMWs, hermes_exec_ack (hermesKV.c:591-674)
// changes a key only through ACKs that match its pending write (ts = last local write's ts, op
// buffer index set): each ORs its sender's bit into ack_bv, and the first one after which ack_bv
// covers the group membership G completes the write (op buffer index := EMPTY, INVALID_WRITE ->
// INVALID, WRITE/REPLAY -> VALID, the read_write_op slot completes; LAST_ACK_SUCCESS from WRITE or
// REPLAY). The ACKs never change the timestamp they match against, so with T[s] = the first
// matching element of sender s (s < 8) and N = G minus the bits already set, that element is
//   j* = max over s in N of T[s] (none if some T[s] is missing), or the first matching element
//        of any sender when N is empty (min of the T[s] and F, the first match from a sender >= 8).
// Without a completion the applier is the first match of a sender < 8 (only those set bits).
// ack_bv ends as ack_bv | the bits of the senders whose T[s] <= j* (every T[s] without a
// completion). Opcodes: ACK_SUCCESS (a LAST_ACK_SUCCESS input stays, except at j*),
// LAST_ACK_SUCCESS for j* from WRITE or REPLAY. k_lookup finishes the non-matching elements, sets T (as max of ~i) and F
// and caches each matching element's ack_bv / state / op buffer index in pf; in k_ack_resolve
// j* (or, without a completion, F) applies the key's meta. T words carry the launch's epoch in
// their upper half, so a word of an earlier launch reads as empty and nothing is cleared (the
// epoch only wraps after 2^29 launches, when the runtime zeroes T with the F words' reset).
// Measured against u32 words with an 11-bit tag and a 1/2048 slice of T zeroed by every ACK
// launch: the slice memset is a kernel of its own (4.6 us), as long as the clear pass it replaced.
enum : uint8_t { kAkMatch = 1 };

__device__ __forceinline__ uint8_t ack_opcode(uint8_t in) { return in == kLastAckSuccess ? in : kAckSuccess; }

__device__ __forceinline__ uint8_t inv_opcode(uint8_t in, bool oog)
{
    return oog ? kInvOutOfGroup : (in == kOpInvAbort || in == kInvOutOfGroup) ? in : kInvSuccess;
}

// Wave-aggregated atomicAdd(&arr[j], 1): one atomic per distinct j in the wave; each active lane
// gets its own ticket. All 64 lanes must call it.
__device__ __forceinline__ uint32_t agg_ticket(uint32_t *arr, uint32_t j, bool active)
{
    const int lane = threadIdx.x & 63;
    uint32_t ticket = 0;
    unsigned long long left = __ballot(active);
    while (left) {
        const int leader = __ffsll((long long)left) - 1;
        const uint32_t jl = __shfl(j, leader, 64);
        const unsigned long long m = left & __ballot(active && j == jl);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&arr[jl], (uint32_t)__popcll(m));
        base = __shfl(base, leader, 64);
        if ((m >> lane) & 1ull) ticket = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        left &= ~m;
    }
    return ticket;
}

// x: the element (global), or its LDS copy
template <int TYPE, int SV>
__device__ __forceinline__ void resolve_elem(const BatchArgs &a, uint32_t i, uint8_t *x, uint8_t *entry,
                                             VCopy *vc = nullptr)
{
    Ctx c = make_ctx(a);
    c.vc = vc;
    uint8_t *xg;
    uint8_t idx;
    elem_at(a, i, xg, idx, c);
    Meta m;
    meta_load(entry, m);
    Meta t = m;
    dispatch<SV>(TYPE, x, entry, idx, t, c);
    if (a.error_flags && !meta_equal(t, m)) atomicOr(a.error_flags, 1u);
}

// ------------------------------------------------------------------ k_lookup (+ round 0 candidates)
// Four lanes per element: each lane reads 16 bytes (two slots) of the element's 64-byte bucket,
// so one load instruction covers a whole bucket line per element. Slots are searched in the
// reference's order (first tag match wins, hermesKV.c:954-975). Each lane group carries
// kLookupPair elements through the three dependent loads (op header, bucket, log line) side by
// side, so twice as many loads are in flight per wave. A hit that would mutate its key's meta as
// it stands (S_0) offers itself as round 0's first candidate. The key compare and the meta load
// together once the slot is known; a candidate then loads its F word, which filters the offer (a
// hot key's later candidates see a smaller F and issue no atomic). Non-candidates never touch F:
// the batch is bound by random 64-B lines, and one less per element beats the shorter dependence
// chain of loading F beside the meta. The launch is split: a short head over the
// first kLookupHead elements gives every hot key a small F first, because at the start of one big
// launch some 10^5 elements are in flight before any F is set, and a hot key's candidates among
// them would all reach its F word (atomics on one address serialise).
//
// VAL batches finish here: hermes_exec_val (hermesKV.c:676-703) never changes a timestamp, so
// every VAL of a launch compares against its key's timestamp at launch start, sets VALID iff they
// match and reports VAL_SUCCESS whatever the state. The VALs of a key commute, and the matching
// ones all store the same state byte.
// esz (a multiple of 8) bytes between 8-byte aligned buffers, 16 B per access
__device__ __forceinline__ void copy_elem(uint8_t *dst, const uint8_t *src, int32_t esz)
{
    for (int32_t o = 0; o + 16 <= esz; o += 16)
        *reinterpret_cast<U64x2 *>(dst + o) = *reinterpret_cast<const U64x2 *>(src + o);
    if (esz & 8) *reinterpret_cast<uint64_t *>(dst + esz - 8) = *reinterpret_cast<const uint64_t *>(src + esz - 8);
}

// bytes 8..15 of an op after its refill patch (second patch word pb, see patch_valid): opcode,
// ST_NEW, val_len; the timestamp (bytes 11..15) kept unless the patch resets it
__device__ __forceinline__ uint64_t patched_hdr(uint64_t h, uint64_t pb)
{
    const bool reset = ((pb >> 40) & 0xFFu) != 0;
    const uint64_t low = (pb & 0xFFu) | ((uint64_t)kNew << 8) | (((pb >> 8) & 0xFFu) << 16);
    return reset ? low : (low | (h & ~0xFFFFFFull));
}

// Local launches with RMWs: how a round-0 candidate (would_mutate against S_0) changes its key, from its
// header word h (bytes 8..15) and S_0 -- bits 0..1: 1 update_actions (a PUT, or an RMW from VALID;
// hermesKV.c:100-141), 2 a write replay (a GET, or an RMW from INVALID: :155-194), 3 anything else (an
// in-progress RMW's abort); bit 2 the RMW flag; bits 8..15 the op's val_len byte. The first two leave the
// key in an absorbing state for the rest of the launch (WRITE or REPLAY with the op buffer index set: every
// later GET, PUT and RMW stalls, and no in-progress RMW matches the new last-local-write timestamp), so the
// elements after F resolve against S_1 (after_first_rmw) in k_resolve0_direct instead of later rounds.
enum : uint16_t { kFkWrite = 1, kFkReplay = 2, kFkOther = 3 };
__device__ __forceinline__ uint16_t fk_kind(uint64_t h, const Meta &m0)
{
    const uint8_t oc = (uint8_t)h, st = (uint8_t)(h >> 8);
    uint16_t k = kFkOther;
    if (oc == kOpPut) k = kFkWrite;
    else if (oc == kOpGet) k = kFkReplay;
    else if (oc == kOpRmw && st != kInProgressRmw) k = m_state(m0) == kValid ? kFkWrite : kFkReplay;
    return (uint16_t)(k | (oc == kOpRmw ? 4u : 0u) | (((h >> 16) & 0xFFu) << 8));
}
// S_1 after F (kind fk, at batch index idx) from S_0, as update_actions / write_replay leave it
__device__ __forceinline__ Meta after_first_rmw(const BatchArgs &a, const Meta &m0, uint16_t fk, uint8_t idx)
{
    Meta m = m0;
    if ((fk & 3u) == kFkWrite) {
        const uint8_t rmw_flag = (fk >> 2) & 1u;
        m_set_val_len(m, (uint8_t)(((uint8_t)(fk >> 8) >> a.g.shift) + kOpMetaSize));
        m_set_rmw(m, rmw_flag);
        m_set_state(m, kWrite);
        m_set_obi(m, idx);
        const uint32_t step = (!a.g.rmw_enabled || rmw_flag == 1) ? 2u : 4u;
        const uint8_t node = (uint8_t)a.g.machine_id;
        m.llw_ver = m.ver + step;
        m.llw_cid = node;
        m_set_ack_bv(m, a.w_ack_init);
        m.ver += step;
        m_set_cid(m, node);
    } else {
        m_set_state(m, kReplay);
        m_set_obi(m, idx);
        m.llw_ver = m.ver;
        m.llw_cid = m_cid(m);
        m_set_ack_bv(m, a.w_ack_init);
    }
    return m;
}

constexpr int64_t kLookupHead = 8192;

template <bool IL = false>
__global__ __launch_bounds__(256) void k_lookup(BatchArgs a, int64_t i_begin, int64_t i_end)
{
    constexpr int P = 1;   // elements per lane group (launch_rounds has the measurements)
    const int q = threadIdx.x & 3;
    const int lane = threadIdx.x & 63;
    const int gbase = lane & ~3;
    if (i_begin == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kCtrFbM] = 0;
        a.ctr[kCtrFbL] = 0;
    }
    const bool vals_direct = a.type == kVals;
    int64_t gi[P];
    uint64_t key[P], hdr[P], tail[P];
    int probe[P];
    bool patched[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        gi[k] = i_begin + ((int64_t)blockIdx.x * P + k) * 64 + (threadIdx.x >> 2);
        uint64_t kk = 0, hh = 0;
        int p = 0;
        patched[k] = false;
        tail[k] = 0;
        if (gi[k] < i_end && q == 0) {
            const int32_t b = (int32_t)(gi[k] / a.stride);
            const int32_t idx = (int32_t)(gi[k] - (int64_t)b * a.stride);
            const bool counted = a.counts == nullptr || idx < a.counts[b];
            if (a.hx) {
                // patch_in_resolve: the element as its patch makes it (k_resolve0_direct writes the op), and
                // its op's last word -- on the line of the next op's header, which the next lane group reads
                const uint8_t *x = a.elems + gi[k] * a.esz;
                const U64x2 h = *reinterpret_cast<const U64x2 *>(x);
                const U64x2 pt = *reinterpret_cast<const U64x2 *>(a.patch + gi[k] * 16);
                tail[k] = *reinterpret_cast<const uint64_t *>(x + a.esz - 8);
                patched[k] = patch_valid(pt.b);
                kk = patched[k] ? pt.a : h.a;
                hh = patched[k] ? patched_hdr(h.b, pt.b) : h.b;
            }
            if (counted) {
                if (!a.hx) {
                    const U64x2 h = *reinterpret_cast<const U64x2 *>(a.elems + gi[k] * a.esz);
                    kk = h.a;
                    hh = h.b;
                }
                if (skip_elem_os(a.type, (uint8_t)hh, (uint8_t)(hh >> 8))) {
                    if (a.type == kInvs && a.ns_idx) {
                        int64_t start;  // packed: a search, for the rare membership-change INVs only
                        const int32_t bb = a.offsets ? batch_of(a, gi[k], start) : b;
                        atomicMax(&a.ns_idx[bb], a.offsets ? (int32_t)(gi[k] - start) : idx);
                    }
                } else {
                    p = 1;
                }
            }
        }
        key[k] = kk;
        hdr[k] = hh;
        probe[k] = p;
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int p = __shfl(probe[k], 0, 4);
        const uint64_t kk = __shfl(key[k], 0, 4);
        probe[k] = p;
        key[k] = kk;
    }
    // bucket, then the log line (lookup_pair: four lanes per element, 16 B each)
    bool ok[P];
    uint64_t phys[P], ekey[P];
    Meta m0[P];
    U64x2 ln[P];
    uint8_t *home[P];
    {
        bool pr[P];
        uint4 l4[P];
#pragma unroll
        for (int k = 0; k < P; ++k) pr[k] = probe[k] != 0;
        lookup_pair<P, IL>(a, key, pr, q, gbase, ok, phys, l4, home);
#pragma unroll
        for (int k = 0; k < P; ++k)
            ln[k] = U64x2{(uint64_t)l4[k].x | ((uint64_t)l4[k].y << 32), (uint64_t)l4[k].z | ((uint64_t)l4[k].w << 32)};
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        ekey[k] = __shfl(ln[k].b, 0, 4);
        const uint64_t w45 = __shfl(ln[k].a, 1, 4), w67 = __shfl(ln[k].b, 1, 4);
        const uint32_t b32 = (uint32_t)__shfl(ln[k].a, 2, 4) & 0xFFu;
        m0[k].w4 = (uint32_t)w45;
        m0[k].w5 = (uint32_t)(w45 >> 32);
        m0[k].ver = (uint32_t)w67;
        m0[k].llw_cid = (uint8_t)(w67 >> 32);
        m0[k].llw_ver = (uint32_t)(w67 >> 40) | (b32 << 24);
    }
    if (q != 0) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (gi[k] >= i_end) continue;
        uint8_t *x = a.elems + gi[k] * a.esz;
        uint32_t e = kNone;
        uint8_t ifl = 0;
        if (ok[k] && ekey[k] == key[k]) {
            e = (uint32_t)(phys[k] / a.g.entry_unit);
            uint8_t *entry = IL ? home[k] : a.log + phys[k];
            if (vals_direct) {
                const uint64_t its = pack_ts((uint32_t)(hdr[k] >> 32), (uint8_t)(hdr[k] >> 24));
                if (its == pack_ts(m0[k].ver, m_cid(m0[k])) && m_state(m0[k]) != kValid) entry[kEntryMetaOff] = kValid;
                x[8] = kValSuccess;
            } else if (a.ack_direct) {
                const uint64_t ats = pack_ts((uint32_t)(hdr[k] >> 32), (uint8_t)(hdr[k] >> 24));
                if (ats != pack_ts(m0[k].llw_ver, m0[k].llw_cid) || m_obi(m0[k]) == kObiEmpty) {
                    x[8] = ack_opcode((uint8_t)hdr[k]);
                } else {
                    ifl = kAkMatch;
                    const uint32_t w = fw_index(a, phys[k]);
                    const uint8_t snd = (uint8_t)(hdr[k] >> 8);
                    // F: the first match of a sender without a T word, or of any sender when the
                    // quorum is complete already (the first match then completes)
                    if (snd >= 8 || (uint8_t)(a.g_membership & ~m_ack_bv(m0[k])) == 0)
                        offer(a.fw + w, a.rtag0, (uint32_t)gi[k]);
                    if (snd < 8) {  // tagged with the launch: no clearing between launches
                        unsigned long long *t = a.ft + (size_t)w * 8 + snd;
                        const unsigned long long tv = ((unsigned long long)(a.rtag0 >> 3) << 32) | (0xFFFFFFFFu - (uint32_t)gi[k]);
                        if (tv > __hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(t, tv);
                    }
                    a.pf[gi[k]] = (uint32_t)m_ack_bv(m0[k]) | ((uint32_t)m_state(m0[k]) << 8) | ((uint32_t)m_obi(m0[k]) << 16);
                }
            } else if (a.inv_direct) {
                const uint64_t its = pack_ts((uint32_t)(hdr[k] >> 32), (uint8_t)(hdr[k] >> 24));
                const uint64_t cur = pack_ts(m0[k].ver, m_cid(m0[k]));
                if (its < cur) {
                    x[8] = inv_opcode((uint8_t)hdr[k], false);
                } else if (its == cur) {
                    ifl = kIvEq | (m_state(m0[k]) == kWrite ? kIvWrite : 0);
                } else {
                    ifl = kIvRaise;
                    a.pf[gi[k]] = 0;  // "B is not A" flag, should this element be A
                    const uint32_t w = fw_index(a, phys[k]);
                    const unsigned long long xv = (its << 24) | (0x7FFFFFull - (uint64_t)gi[k]);
                    if (xv > __hip_atomic_load(a.fx + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.fx + w, xv);
                    if (m_state(m0[k]) == kWrite) offer(a.fw + w, a.rtag0, (uint32_t)gi[k]);
                }
            } else {
                uint64_t h2[2] = {0, hdr[k]};
                Ctx c = make_ctx(a);
                if (would_mutate(a.type, reinterpret_cast<const uint8_t *>(h2), m0[k], c)) {
                    if (a.fk) a.fk[gi[k]] = fk_kind(hdr[k], m0[k]);
                    const unsigned long long vv = ((unsigned long long)(~a.rtag0) << 32) | (uint32_t)gi[k];
                    unsigned long long *fw = a.fw + fw_index(a, phys[k]);
                    if (vv < __hip_atomic_load(fw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(fw, vv);
                    // the seqlock byte is free at batch boundaries (concur_ctrl.h: the lock is held
                    // only inside one exec call): it tells k_resolve0 which keys have a candidate,
                    // so the others skip the F word; the key's commit clears it
                    if ((uint8_t)(m0[k].w5 >> 16) != a.ltag) entry[kEntryMetaOff + 4] = a.ltag;
                }
            }
        }
        if (patched[k]) {   // k_resolve0_direct writes the op's header from this word
            const uint64_t h = probe[k] && e == kNone ? (hdr[k] & ~0xFF00ull) | ((uint64_t)kMiss << 8) : hdr[k];
            *reinterpret_cast<U64x2 *>(a.hx + 2 * gi[k]) = U64x2{h, tail[k]};
        } else if (probe[k] && e == kNone) {
            x[9] = kMiss;
        }
        a.ent[gi[k]] = e;
        if (a.inv_direct || a.ack_direct) a.st[gi[k]] = ifl;
    }
}

// INV direct path: opcodes of the elements at or above ts_0, A marks itself, the other elements
// with ts M (or, without a raise, all of them) set Y. The load before each atomicMax filters the
// offers of a key with many INVs (Y only rises).
__global__ __launch_bounds__(256) void k_inv_resolve(BatchArgs a, int64_t i_begin, int64_t i_end)
{
    const int64_t i = i_begin + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= i_end) return;
    const uint8_t fl = a.st[i];
    if (fl == 0) return;
    const uint32_t w = fw_index(a, phys_of(a, a.ent[i]));
    uint8_t *x = a.elems + i * a.esz;
    const uint64_t hdr = *reinterpret_cast<const uint64_t *>(x + 8);
    const uint64_t its = pack_ts((uint32_t)(hdr >> 32), (uint8_t)(hdr >> 24));
    const unsigned long long X = a.fx[w];  // M and A are final (k_lookup)
    bool oog = false, y = false;
    if (X != 0) {  // some element raises the key's ts
        // in state WRITE, an element at ts_0 is out of group until the first raise P (offered by
        // every raising element of a key in state WRITE, so it exists)
        if (fl & kIvWrite) oog = (uint32_t)i < first_cand(a.fw[w], a.rtag0);
        const uint32_t ia = 0x7FFFFFu - (uint32_t)(X & 0x7FFFFFu);
        if ((uint32_t)i == ia) {
            a.st[i] = kIvApply;
            a.mem[i] = X;
        } else if (its == (uint64_t)(X >> 24)) {
            y = true;
            if (a.pf[ia] == 0) a.pf[ia] = 1;  // every writer stores the same value
        }
    } else {       // no raise: every flagged element of the key is at ts_0, B applies
        oog = (fl & kIvWrite) != 0;
        y = true;
        a.st[i] = kIvCand;
    }
    x[8] = inv_opcode((uint8_t)hdr, oog);
    if (y) {
        const unsigned long long yv = (unsigned long long)i + 1;
        if (yv > __hip_atomic_load(a.fy + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.fy + w, yv);
    }
}

// A of a raising key applies the key's meta to a 64-B entry (31-B values): entry bytes 16..63
// (meta, value) and the element's bytes 16..63 (flags, value) move as three 16-B words each, the
// new entry image is put together in registers.
__device__ __forceinline__ void inv_apply64(const BatchArgs &a, int64_t i, uint32_t w, uint8_t *entry,
                                            unsigned long long X)
{
    union Img {
        U64x2 q[3];
        uint64_t d[6];
    };
    Img en, el;
    const U64x2 *pe = reinterpret_cast<const U64x2 *>(entry + 16);
    const U64x2 *px = reinterpret_cast<const U64x2 *>(a.elems + i * a.esz + 16);
#pragma unroll
    for (int k = 0; k < 3; ++k) en.q[k] = pe[k];
    el.q[0] = px[0];  // the 56-B element ends at image byte 40: bytes 16..55 only
    el.q[1] = px[1];
    el.d[4] = *reinterpret_cast<const uint64_t *>(px + 2);
    el.d[5] = 0;
    int64_t b = i;
    if (a.pf[i]) {  // B is not A
        b = (int64_t)a.fy[w] - 1;
        a.fy[w] = 0;
    }
    const uint8_t lw = a.elems[b * a.esz + 9];
    Meta m;
    m.w4 = (uint32_t)en.d[0];
    m.w5 = (uint32_t)(en.d[0] >> 32);
    m.ver = (uint32_t)en.d[1];
    m.llw_cid = (uint8_t)(en.d[1] >> 32);
    m.llw_ver = (uint32_t)(en.d[1] >> 40) | ((uint32_t)(en.d[2] & 0xFFu) << 24);
    const uint64_t M = X >> 24;
    const uint8_t st = m_state(m);
    if (st == kValid) m_set_state(m, kInvalid);
    else if (st == kWrite || st == kReplay) m_set_state(m, kInvalidWrite);
    m_set_val_len(m, (uint8_t)a.g.kvs_value);
    m_set_rmw(m, (uint8_t)(el.d[0] & 1u));  // element byte 16: RMW_flag
    m_set_lwid(m, lw);
    m.ver = (uint32_t)(M >> 8);
    m_set_cid(m, (uint8_t)M);
    // value: element bytes 18..48 -> entry bytes 33..63, i.e. image byte 2 + k -> 17 + k: the
    // element image shifted up by 15 bytes = 120 bits (one word and 56 bits)
    uint64_t v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t lo = k >= 2 ? el.d[k - 2] : 0, hi = k >= 1 ? el.d[k - 1] : 0;
        v[k] = (hi << 56) | (lo >> 8);
    }
    // bytes 0..15 of the image: meta (seqlock byte free), byte 16: llw_ver's top byte, 17..47: value
    Img out;
    out.d[0] = (uint64_t)m.w4 | ((uint64_t)(m.w5 & 0xFF00FFFFu) << 32);
    out.d[1] = (uint64_t)m.ver | ((uint64_t)m.llw_cid << 32) | ((uint64_t)m.llw_ver << 40);
    out.d[2] = (uint64_t)(uint8_t)(m.llw_ver >> 24) | (v[2] & ~0xFFull);
    out.d[3] = v[3];
    out.d[4] = v[4];
    out.d[5] = v[5];
    U64x2 *po = reinterpret_cast<U64x2 *>(entry + 16);
#pragma unroll
    for (int k = 0; k < 3; ++k) po[k] = out.q[k];
    a.fx[w] = 0;
}

// INV direct path: A (or, without a raise, B) applies its key's meta and clears X and Y.
template <int SV>
__global__ __launch_bounds__(256) void k_inv_commit(BatchArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t fl = a.st[i];
    if (fl != kIvApply && fl != kIvCand) return;
    const uint32_t e = a.ent[i];
    const uint32_t w = fw_index(a, phys_of(a, e));
    int64_t b = i;  // B
    if (fl == kIvCand) {
        if (a.fy[w] != (unsigned long long)i + 1) return;
        a.fy[w] = 0;
    }
    uint8_t *entry = entry_of(a, e);
    if (SV == 31 && fl == kIvApply) {  // 64-B entries: bytes 16..63 in and out as three 16-B words
        inv_apply64(a, i, w, entry, a.mem[i]);
        return;
    }
    Meta m;
    meta_load(entry, m);
    if (fl == kIvApply) {
        const unsigned long long X = a.mem[i];
        if (a.pf[i]) {
            b = (int64_t)a.fy[w] - 1;
            a.fy[w] = 0;
        }
        const uint8_t *xa = a.elems + i * a.esz;
        const uint64_t M = X >> 24;
        const uint8_t st = m_state(m);
        if (st == kValid) m_set_state(m, kInvalid);
        else if (st == kWrite || st == kReplay) m_set_state(m, kInvalidWrite);
        m_set_val_len(m, (uint8_t)a.g.kvs_value);
        m_set_rmw(m, e_rmw(xa));
        copy_value<SV>(entry + kEntryValueOff, xa + kOpValueOff, a.g.st_value);
        m.ver = (uint32_t)(M >> 8);
        m_set_cid(m, (uint8_t)M);
        a.fx[w] = 0;
    }
    m_set_lwid(m, a.elems[b * a.esz + 9]);
    meta_store(entry, m);
}

// ACK direct path: each matching element finds j*; j* (or, without a completion, F) applies the
// key's meta and completes the read_write_op slot. Nothing else reads the entry in this pass (the
// others use the cached S_0 fields), so the applier writes it here.
__global__ __launch_bounds__(256) void k_ack_resolve(BatchArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n || a.st[i] != kAkMatch) return;
    const uint32_t e = a.ent[i];
    const uint32_t w = fw_index(a, phys_of(a, e));
    const uint32_t c0 = a.pf[i];
    const uint8_t bv0 = (uint8_t)c0, st0 = (uint8_t)(c0 >> 8), obi0 = (uint8_t)(c0 >> 16);
    const U64x2 *tp = reinterpret_cast<const U64x2 *>(a.ft + (size_t)w * 8);
    uint32_t tv[8];  // 0xFFFFFFFF - (first match of the sender), 0: none in this launch
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const U64x2 p = tp[h];
        tv[2 * h] = (uint32_t)(p.a >> 32) == (a.rtag0 >> 3) ? (uint32_t)p.a : 0u;
        tv[2 * h + 1] = (uint32_t)(p.b >> 32) == (a.rtag0 >> 3) ? (uint32_t)p.b : 0u;
    }
    const uint8_t need = (uint8_t)(a.g_membership & ~bv0);
    // the first match of senders 0..7 (min T), and of any sender (with F; F is offered only by
    // matches from senders >= 8, or by every match when need is empty)
    uint32_t f = kNone;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (tv[s] != 0) f = min(f, 0xFFFFFFFFu - tv[s]);
    uint32_t js = kNone;  // j*
    if (need == 0) {
        js = min(f, first_cand(a.fw[w], a.rtag0));  // F is read only here
    } else {
        uint32_t mx = 0;
        bool all = true;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (!((need >> s) & 1u)) continue;
            if (tv[s] == 0) all = false;
            else mx = max(mx, 0xFFFFFFFFu - tv[s]);
        }
        if (all) js = mx;
    }
    uint8_t *x = a.elems + i * a.esz;
    const bool done = (uint32_t)i == js;
    const bool wr = st0 == kWrite || st0 == kReplay;
    // j* overwrites the opcode (LAST_ACK_SUCCESS, or LAST_ACK_NO_BCAST -> ACK_SUCCESS), even a
    // LAST_ACK_SUCCESS input; the others keep a LAST_ACK_SUCCESS input
    x[8] = done ? (wr ? kLastAckSuccess : kAckSuccess) : ack_opcode(x[8]);
    if (!(done || (js == kNone && (uint32_t)i == f))) return;
    // the applier: ack_bv, and with a completion the state, op buffer index and read_write_op
    uint8_t bv = bv0;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (tv[s] != 0 && (js == kNone || 0xFFFFFFFFu - tv[s] <= js)) bv |= (uint8_t)(1u << s);
    uint8_t *entry = entry_of(a, e);
    Meta m;
    meta_load(entry, m);
    m_set_ack_bv(m, bv);
    if (done) {
        if (st0 == kInvalidWrite) m_set_state(m, kInvalid);
        else if (wr) m_set_state(m, kValid);
        else if (st0 != kValid && st0 != kInvalid && a.error_flags) atomicOr(a.error_flags, 2u);
        m_set_obi(m, kObiEmpty);
        if (a.rw) {
            int64_t start;
            const int64_t b = batch_of(a, i, start);
            uint8_t *rw = a.rw + b * a.rw_stride + (size_t)obi0 * a.g.op_size;
            const uint8_t oc = rw[8];
            const uint8_t ns = oc == kOpGet ? kNew : oc == kOpPut ? kPutComplete : oc == kOpRmw ? kRmwComplete : rw[9];
            rw[9] = ns;
            if (a.rws) a.rws[b * (a.rw_stride / a.g.op_size) + obi0] = ns;
        }
    }
    meta_store(entry, m);
}

// ------------------------------------------------------------------ rounds (passes over all elements)
// Candidates of round r >= 1: pending elements against S_r, which round r-1's first candidate left
// in its shadow. Aggregated per key in LDS over kCandPer * 256 elements (see k_lookup).
constexpr int kCandPer = 4;
constexpr int kCandSlots = 2048;  // >= 2 * kCandPer * 256: the probe always ends
template <int TYPE>
__global__ __launch_bounds__(256) void k_cand(BatchArgs a, int r)
{
    __shared__ uint32_t lk[kCandSlots], lv[kCandSlots];
    for (int j = threadIdx.x; j < kCandSlots; j += 256) {
        lk[j] = kNone;
        lv[j] = kNone;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * 256 * kCandPer;
#pragma unroll
    for (int k = 0; k < kCandPer; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        if (i >= a.n) break;
        if (a.st[i] != kStPend) continue;
        Meta m;
        meta_load(shadow_of(a, a.pf[i]), m);
        uint64_t h2[2] = {0, ld64(a.elems + i * a.esz + 8)};
        Ctx c = make_ctx(a);
        if (!would_mutate(TYPE, reinterpret_cast<const uint8_t *>(h2), m, c)) continue;
        const uint32_t fi = fw_index(a, phys_of(a, a.ent[i]));
        uint32_t h = (fi * 0x9E3779B1u) >> 21;
        for (;;) {
            const uint32_t old = atomicCAS(&lk[h], kNone, fi);
            if (old == kNone || old == fi) {
                atomicMin(&lv[h], (uint32_t)i);
                break;
            }
            h = (h + 1) & (kCandSlots - 1);
        }
    }
    __syncthreads();
    const uint32_t rtag = a.rtag0 + (uint32_t)r;
    for (int j = threadIdx.x; j < kCandSlots; j += 256)
        if (lk[j] != kNone) offer(a.fw + lk[j], rtag, lv[j]);
}

// Round 0's resolve over every element, on LDS copies of the block's contiguous op slab (copied
// in and out with 16-B accesses, so the byte-wise result writes never reach memory one by one).
// Before F_0 (or no candidate) -> resolved now; F_0 -> applied to its shadow; after -> pending.
template <int TYPE, int SV, int BP>
__global__ __launch_bounds__(BP) void k_resolve0(BatchArgs a)
{
    extern __shared__ uint4 sops[];
    // 64-B entries: each thread reads bytes 16..63 (meta + value) in three 16-B accesses; the meta
    // comes from registers, the value from the thread's LDS copy
    constexpr bool kStage = SV == 31;
    __shared__ U64x2 sent[kStage ? 3 * BP : 1];
    const int64_t i0 = (int64_t)blockIdx.x * BP;
    const int cnt = a.n - i0 < BP ? (int)(a.n - i0) : BP;
    // the element's entry id and meta load while the block copies its op slab in
    const uint32_t e = (int)threadIdx.x < cnt ? a.ent[i0 + threadIdx.x] : kNone;
    Meta m{};
    if (e != kNone) {
        if (kStage) {
            const U64x2 *p = reinterpret_cast<const U64x2 *>(entry_of(a, e));
            const U64x2 l1 = p[1], l2 = p[2], l3 = p[3];
            m.w4 = (uint32_t)l1.a;
            m.w5 = (uint32_t)(l1.a >> 32);
            m.ver = (uint32_t)l1.b;
            m.llw_cid = (uint8_t)(l1.b >> 32);
            m.llw_ver = (uint32_t)(l1.b >> 40) | ((uint32_t)(l2.a & 0xFFu) << 24);
            sent[3 * threadIdx.x] = l1;
            sent[3 * threadIdx.x + 1] = l2;
            sent[3 * threadIdx.x + 2] = l3;
        } else {
            meta_load(entry_of(a, e), m);
        }
    }
    // what the non-mutating elements read the entry value from (bytes below 16 are never read)
    uint8_t *rentry = kStage ? reinterpret_cast<uint8_t *>(&sent[3 * threadIdx.x]) - 16 : entry_of(a, e);
    const uint32_t bytes = (uint32_t)cnt * (uint32_t)a.esz;  // a multiple of 8
    // big ops (56 + 64 c bytes for c extra cache lines: 312 B at c = 4, 1080 B at most): only the elements that
    // hit move through LDS (message slabs are mostly padding); 8-B words, each inside one element
    constexpr bool kLive = BP == 128;
    __shared__ uint8_t live[kLive ? BP : 1];
    const uint32_t ew = (uint32_t)a.esz / 8u;
    if (kLive) {
        live[threadIdx.x] = e != kNone;
        __syncthreads();
        const uint64_t *src = reinterpret_cast<const uint64_t *>(a.elems + i0 * a.esz);
        uint64_t *s8 = reinterpret_cast<uint64_t *>(sops);
        for (uint32_t w = threadIdx.x; w < bytes / 8; w += BP)
            if (live[w / ew]) s8[w] = src[w];
    } else {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.elems + i0 * a.esz);
        for (uint32_t w = threadIdx.x; w < bytes / 16; w += BP) sops[w] = src[w];
        if ((bytes & 8) && threadIdx.x == 0)
            reinterpret_cast<uint64_t *>(sops)[bytes / 8 - 1] = reinterpret_cast<const uint64_t *>(src)[bytes / 8 - 1];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < cnt) {
        const int64_t i = i0 + t;
        uint8_t st = kStDone;
        if (e != kNone) {
            // only keys flagged by k_lookup can have a first candidate
            const uint32_t f = (uint8_t)(m.w5 >> 16) == a.ltag ? first_cand(*fw_of(a, e), a.rtag0) : kNone;
            if (f == kNone || (uint32_t)i < f) {
                Ctx c = make_ctx(a);
                uint8_t *xg;
                uint8_t idx;
                elem_at(a, (uint32_t)i, xg, idx, c);
                Meta tm = m;
                dispatch<SV>(TYPE, reinterpret_cast<uint8_t *>(sops) + (uint32_t)t * a.esz, rentry, idx, tm, c);
                if (a.error_flags && !meta_equal(tm, m)) atomicOr(a.error_flags, 1u);
            } else if ((uint32_t)i == f) {
                apply_to_shadow<TYPE, SV>(a, reinterpret_cast<uint8_t *>(sops) + (uint32_t)t * a.esz, (uint32_t)i,
                                          entry_of(a, e));
                st = kStCommit;
            } else if (a.rounds == 0) {  // after the key's only mutation: absorbing state
                Ctx c = make_ctx(a);
                uint8_t *xg;
                uint8_t idx;
                elem_at(a, (uint32_t)i, xg, idx, c);
                const Meta m1 = after_first<TYPE>(a, m, f, 0);
                Meta tm = m1;
                dispatch<SV>(TYPE, reinterpret_cast<uint8_t *>(sops) + (uint32_t)t * a.esz, rentry, idx, tm, c);
                if (a.error_flags && !meta_equal(tm, m1)) atomicOr(a.error_flags, 1u);
            } else {
                a.pf[i] = f;
                st = kStPend;
            }
        }
        a.st[i] = st;
        // big ops move through LDS only when they hit (kLive); the others are in memory unchanged
        note_state(a, i, kLive && e == kNone ? a.elems + i * a.esz
                                              : reinterpret_cast<const uint8_t *>(sops) + (uint32_t)t * a.esz);
    }
    __syncthreads();
    if (kLive) {
        uint64_t *dst = reinterpret_cast<uint64_t *>(a.elems + i0 * a.esz);
        const uint64_t *s8 = reinterpret_cast<const uint64_t *>(sops);
        for (uint32_t w = threadIdx.x; w < bytes / 8; w += BP)
            if (live[w / ew]) dst[w] = s8[w];
        return;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(a.elems + i0 * a.esz);
    for (uint32_t w = threadIdx.x; w < bytes / 16; w += BP) dst[w] = sops[w];
    if ((bytes & 8) && threadIdx.x == 0)
        reinterpret_cast<uint64_t *>(dst)[bytes / 8 - 1] = reinterpret_cast<const uint64_t *>(sops)[bytes / 8 - 1];
}

// k_resolve0 for big ops (any op of more than 64 B: 56 + 64 c bytes, 312 B at c = 4) in place: one thread per
// element on its global copy, no LDS, so occupancy is bound by registers instead of by an op's bytes of LDS per
// element (local and ACK launches). Values of at most 320 B are copied, and a key's first candidate applied to
// its shadow, by the whole wave; larger ones by their own lane (the wave copies hold 64 lanes x 5 bytes, and
// apply_to_shadow_wave's block copies were laid out for entries of a few lanes)
// The value copies the wave's exec calls recorded (Ctx::vc), made by the whole wave: byte k of a
// value by lane k % 64, so each instruction moves 64 consecutive bytes. kVcBatch values at a time:
// all their loads are issued before the first store, so a wave waits one memory latency per
// kVcBatch values instead of one per value. Every lane of the wave
// calls it.
constexpr int kVcBatch = 4;
template <int VB>
__device__ __forceinline__ void wave_value_copies_n(const VCopy &v, uint32_t n)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(v.dst != nullptr);
    while (todo) {
        uint8_t *dp[VB];
        const uint8_t *sp[VB];
#pragma unroll
        for (int u = 0; u < VB; ++u) {   // the next VB recorded copies (todo is the same in every lane)
            dp[u] = nullptr;
            sp[u] = nullptr;
            if (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint64_t d = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(uintptr_t)v.dst, j, 64) |
                                   ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uintptr_t)v.dst >> 32), j, 64) << 32);
                const uint64_t s = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(uintptr_t)v.src, j, 64) |
                                   ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uintptr_t)v.src >> 32), j, 64) << 32);
                dp[u] = reinterpret_cast<uint8_t *>(d);
                sp[u] = reinterpret_cast<const uint8_t *>(s);
            }
        }
        uint8_t b[VB][5];
#pragma unroll
        for (int u = 0; u < VB; ++u)
#pragma unroll
            for (int r = 0; r < 5; ++r) {   // values up to 320 B; all loads before the stores
                const uint32_t k = (uint32_t)lane + 64u * r;
                b[u][r] = sp[u] && k < n ? sp[u][k] : 0;
            }
#pragma unroll
        for (int u = 0; u < VB; ++u)
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const uint32_t k = (uint32_t)lane + 64u * r;
                if (dp[u] && k < n) dp[u][k] = b[u][r];
            }
    }
}

// bytes [lo, hi) of the 8-byte word v to the 8-byte aligned p, in aligned 1/2/4-byte stores (the
// word's other bytes are other fields: op header, entry meta)
__device__ __forceinline__ void store_word_part(uint8_t *p, uint64_t v, uint32_t lo, uint32_t hi)
{
    for (uint32_t b = lo; b < hi;) {
        if ((b & 3) == 0 && b + 4 <= hi) {
            *reinterpret_cast<uint32_t *>(p + b) = (uint32_t)(v >> (8 * b));
            b += 4;
        } else if ((b & 1) == 0 && b + 2 <= hi) {
            *reinterpret_cast<uint16_t *>(p + b) = (uint16_t)(v >> (8 * b));
            b += 2;
        } else {
            p[b] = (uint8_t)(v >> (8 * b));
            b += 1;
        }
    }
}

// wave_value_copies_n by 8-byte words: lane k stores the destination's aligned word k (the two end
// words byte-exact), built from the aligned source words k and k + 1 (the latter from lane k + 1), so
// a 287-byte value is 37 lanes of one load and one store instead of five byte instructions each way
// (the op value sits at byte 18 and the entry value at byte 33, so the two ends differ mod 8). Only
// source words holding a byte of the value are loaded.
template <int VB>
__device__ __forceinline__ void wave_value_words_n(const VCopy &v, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(v.dst != nullptr);
    while (todo) {
        uint8_t *dp[VB];
        const uint8_t *sp[VB];
        uint32_t fl[VB];
#pragma unroll
        for (int u = 0; u < VB; ++u) {
            dp[u] = nullptr;
            sp[u] = nullptr;
            fl[u] = 0;
            if (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint64_t d = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(uintptr_t)v.dst, j, 64) |
                                   ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uintptr_t)v.dst >> 32), j, 64) << 32);
                const uint64_t s = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(uintptr_t)v.src, j, 64) |
                                   ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uintptr_t)v.src >> 32), j, 64) << 32);
                dp[u] = reinterpret_cast<uint8_t *>(d);
                sp[u] = reinterpret_cast<const uint8_t *>(s);
                fl[u] = (uint32_t)__shfl((int)v.fill, j, 64);
            }
        }
        uint64_t w[VB];
#pragma unroll
        for (int u = 0; u < VB; ++u) {   // all loads before the stores
            // destination word k takes the source bytes from base + 8k; aligned source word j is at ab + 8j
            const uintptr_t s = (uintptr_t)sp[u], d0 = (uintptr_t)dp[u] & 7u;
            const uintptr_t ab = (s - d0) & ~(uintptr_t)7;
            const uintptr_t wa = ab + 8u * lane;
            w[u] = 0;
            if (fl[u]) w[u] = 0x0101010101010101ull * (uint8_t)fl[u];   // every word (any shift of it is itself)
            else if (sp[u] && wa + 8 > s && wa < s + n) w[u] = *reinterpret_cast<const uint64_t *>(wa);
        }
#pragma unroll
        for (int u = 0; u < VB; ++u) {
            const uint64_t hi_w = (uint64_t)(uint32_t)__shfl_down((int)(uint32_t)w[u], 1, 64) |
                                  ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(w[u] >> 32), 1, 64) << 32);
            if (!dp[u]) continue;
            const uint32_t d0 = (uint32_t)((uintptr_t)dp[u] & 7u);
            const uint32_t r = (uint32_t)(((uintptr_t)sp[u] - d0) & 7u);
            const uint32_t nw = (d0 + n + 7u) >> 3;
            if (lane >= nw) continue;
            const uint64_t val = r ? (w[u] >> (8 * r)) | (hi_w << (64 - 8 * r)) : w[u];
            uint8_t *dw = dp[u] - d0 + 8u * lane;
            const uint32_t lo = lane == 0 ? d0 : 0u;
            const uint32_t hi = lane == nw - 1 ? d0 + n - 8u * (nw - 1) : 8u;
            if (lo == 0 && hi == 8) *reinterpret_cast<uint64_t *>(dw) = val;
            else store_word_part(dw, val, lo, hi);
        }
    }
}

// by words where the value allows it; values over 496 B take the byte-wise copies
__device__ __forceinline__ void wave_value_copies(const VCopy &v, uint32_t n, int batch)
{
    if (n <= kWaveWordsMaxValue) {
        if (batch == 1) wave_value_words_n<1>(v, n);
        else wave_value_words_n<kVcBatch>(v, n);
        return;
    }
    if (batch == 1) wave_value_copies_n<1>(v, n);
    else wave_value_copies_n<kVcBatch>(v, n);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src)
{
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64) << 32);
}

// Whole-wave copies of `bytes` (a multiple of 8, 8-byte aligned ends) recorded one per lane (dst
// null: none): C = bytes / 16 rounded up lanes per copy move 16 B each, 64 / C copies per
// instruction, and kBcRounds instructions' loads are issued before their stores. Every lane of the
// wave calls it.
constexpr int kBcRounds = 2;
__device__ __forceinline__ void wave_block_copies(uint8_t *dst, const uint8_t *src, uint32_t bytes)
{
    struct __attribute__((aligned(8))) W16 {
        uint64_t a, b;
    };
    const int lane = threadIdx.x & 63;
    const int C = (int)((bytes + 15) / 16);
    unsigned long long todo = __ballot(dst != nullptr);
    if (C > 64) {   // more than 1024 B (1088-B entries): no copy fits one instruction, so the wave strides over
                    // one copy at a time (per below would be 0 and the loop would never take a copy off todo)
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            uint8_t *d = reinterpret_cast<uint8_t *>(shfl_u64((uint64_t)(uintptr_t)dst, j));
            const uint8_t *sa = reinterpret_cast<const uint8_t *>(shfl_u64((uint64_t)(uintptr_t)src, j));
            for (uint32_t o = 16u * (uint32_t)lane; o < bytes; o += 1024u) {
                if (o + 16u > bytes) *reinterpret_cast<uint64_t *>(d + o) = *reinterpret_cast<const uint64_t *>(sa + o);
                else *reinterpret_cast<W16 *>(d + o) = *reinterpret_cast<const W16 *>(sa + o);
            }
        }
        return;
    }
    const int per = 64 / C;
    const int slot = lane / C, ch = lane - slot * C;
    while (todo) {
        W16 v[kBcRounds];
        uint8_t *dp[kBcRounds];
        bool half[kBcRounds];
#pragma unroll
        for (int r = 0; r < kBcRounds; ++r) {
            int mine = -1;
            for (int k = 0; k < per; ++k) {   // this instruction's copies, lane order (todo is uniform)
                if (!todo) break;
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                if (k == slot) mine = j;
            }
            const int sl = mine < 0 ? 0 : mine;
            const uint64_t d = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(uintptr_t)dst, sl, 64) |
                               ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uintptr_t)dst >> 32), sl, 64) << 32);
            const uint64_t sa = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(uintptr_t)src, sl, 64) |
                                ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uintptr_t)src >> 32), sl, 64) << 32);
            dp[r] = mine >= 0 && slot < per ? reinterpret_cast<uint8_t *>(d) + 16 * ch : nullptr;
            half[r] = 16 * ch + 16 > (int)bytes;
            const uint8_t *sp = reinterpret_cast<const uint8_t *>(sa) + 16 * ch;
            v[r] = W16{0, 0};
            if (dp[r]) {
                if (half[r]) v[r].a = *reinterpret_cast<const uint64_t *>(sp);
                else v[r] = *reinterpret_cast<const W16 *>(sp);
            }
        }
#pragma unroll
        for (int r = 0; r < kBcRounds; ++r) {
            if (!dp[r]) continue;
            if (half[r]) *reinterpret_cast<uint64_t *>(dp[r]) = v[r].a;
            else *reinterpret_cast<W16 *>(dp[r]) = v[r];
        }
    }
}

// apply_to_shadow for big entries, by the whole wave (every lane calls it; cand: this lane's element
// is its key's first candidate, src its S_r): the wave copies S_r into the candidates' shadows
// (wave_block_copies), then each candidate runs its exec function on its shadow with the value
// copy recorded in vc (made by wave_value_copies after it), instead of one lane copying 320 + 287
// bytes in dependent steps while the rest of its wave waits.
template <int TYPE, int SV>
__device__ __forceinline__ void apply_to_shadow_wave(const BatchArgs &a, bool cand, uint32_t i, const uint8_t *src,
                                                     VCopy &vc, uint8_t *xl = nullptr, bool use_xl = false)
{
    uint8_t *sh = cand ? shadow_of(a, i) : nullptr;
    wave_block_copies(sh, src, a.g.entry_size);
    __threadfence_block();   // the shadows' bytes before any lane reads or rewrites them
    if (!cand) return;
    Meta m;
    meta_load(src, m);
    Ctx c = make_ctx(a);
    c.vc = &vc;
    uint8_t *xg;
    uint8_t idx;
    elem_at(a, i, xg, idx, c);
    if (use_xl) dispatch<SV>(TYPE, xl, sh, idx, m, c);   // xl: the element's patched copy (k_resolve0_direct)
    else dispatch<SV>(TYPE, xg, sh, idx, m, c);
    meta_store(sh, m);
}

// patch_in_resolve (big local launches with refill patches, a.hx set; launch_batch): k_lookup read each
// patch beside the op's header, so a patched element runs its exec function on a copy of its op's first 24
// bytes in LDS -- key and header word as patched (k_lookup), flags from the patch -- and this pass writes the
// op once: its header from the copy, a write's value fill (a copy with no source to load), the GET values
// the exec functions copy, and the pad bytes after the value from the op's last word (k_lookup), so the op's
// 64-byte blocks are written whole (a block written with holes costs HBM a read-modify-write:
// tools/write_bench.hip). The refill's own pass over the slab (k_refill_st_w) goes, and this pass reads
// no op line: the header came with k_lookup's read, a write's value is the patch's fill byte.
// Ops whose every byte is known (k_resolve0_direct's whole ones: key h0, header h1, flags and fill byte fl, the
// fill, the last word lw; nw 8-byte words) written by the whole wave: (nw + 1) / 2 lanes per op, 16 B each, so
// one store instruction writes 64 / that many ops contiguously. Every lane calls it.
__device__ __forceinline__ void wave_whole_ops(uint8_t *xg, bool whole, uint64_t h0, uint64_t h1, uint32_t fl, uint64_t lw,
                                               uint32_t nw)
{
    const int lane = threadIdx.x & 63;
    const int C = (int)((nw + 1) / 2);
    const int per = 64 / C;
    const int slot = lane / C, ch = lane - slot * C;
    unsigned long long todo = __ballot(whole);
    while (todo) {
        int mine = -1;
        for (int k = 0; k < per; ++k) {   // (todo is the same in every lane)
            if (!todo) break;
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            if (k == slot) mine = j;
        }
        const int sl = mine < 0 ? 0 : mine;
        const uint64_t d = shfl_u64((uint64_t)(uintptr_t)xg, sl), a0 = shfl_u64(h0, sl), a1 = shfl_u64(h1, sl);
        const uint64_t l = shfl_u64(lw, sl);
        const uint32_t f = (uint32_t)__shfl((int)fl, sl, 64);
        if (mine < 0 || slot >= per) continue;
        const uint64_t pat = 0x0101010101010101ull * ((f >> 16) & 0xFFu);
        auto word = [&](uint32_t k) {
            return k == 0 ? a0 : k == 1 ? a1 : k == 2 ? ((uint64_t)(f & 0xFFFFu) | (pat << 16)) : k == nw - 1 ? l : pat;
        };
        const uint32_t k0 = 2u * (uint32_t)ch;
        uint8_t *p = reinterpret_cast<uint8_t *>(d) + 8u * k0;
        if (k0 + 1 < nw) *reinterpret_cast<U64x2 *>(p) = U64x2{word(k0), word(k0 + 1)};
        else *reinterpret_cast<uint64_t *>(p) = word(k0);
    }
}

// waves per SIMD k_resolve0_direct is compiled for (its registers: 512 / waves). At 8 it fits 64 VGPRs
// instead of 127 (4 waves per SIMD): configs[2] fresh 0.736-0.741 -> 0.772-0.782 G ops/s (gpurun_out/r06s;
// in round 5's kernel, before the patches, it was level)
template <int TYPE, int SV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_resolve0_direct(BatchArgs a)
{
    constexpr bool kPir = TYPE == kLocal && SV != 31;
    __shared__ uint64_t sop[kPir ? 256 * 3 : 1];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < a.n;
    const uint32_t e = in ? a.ent[i] : kNone;
    U64x2 pt{0, 0}, hw{0, 0};
    if (kPir && a.hx && in) {   // beside the entry id: one trip
        pt = *reinterpret_cast<const U64x2 *>(a.patch + i * 16);
        hw = *reinterpret_cast<const U64x2 *>(a.hx + 2 * i);
    }
    const bool pd = kPir && a.hx && in && patch_valid(pt.b);
    const uint32_t fb = (uint32_t)(pt.b >> 32) & 0xFFu;   // a patched element's value fill byte (0: none)
    uint64_t *cop = &sop[kPir ? threadIdx.x * 3 : 0];
    if (pd) {
        cop[0] = pt.a;
        cop[1] = hw.a;
        cop[2] = ((pt.b >> 16) & 0xFFFFull) | (fb ? (0x0101010101010101ull * fb) << 16 : 0ull);
    }
    uint8_t st = kStDone;
    uint8_t *xg = nullptr;
    uint8_t idx = 0;
    Ctx c = make_ctx(a);
    // big values: the exec calls record their value copy, made by the whole wave afterwards (the
    // key's entry is not written in this pass -- its first candidate writes its own shadow -- and
    // the op is this lane's own)
    VCopy vc{nullptr, nullptr};
    if (SV != 31 && a.g.st_value <= 320) c.vc = &vc;
    // a key's first candidate applies itself to its shadow by the whole wave (apply_to_shadow_wave)
    const bool wave_shadow = SV != 31 && a.g.st_value <= 320;
    bool cand = false;
    if (in) elem_at(a, (uint32_t)i, xg, idx, c);
    // the op the exec functions see: the LDS copy of a patched one, else the op (two calls, so each keeps
    // its address space instead of flat accesses)
    uint8_t *xl = reinterpret_cast<uint8_t *>(cop);
    if (e != kNone) {
        Meta m;
        meta_load(entry_of(a, e), m);
        const uint32_t f = (uint8_t)(m.w5 >> 16) == a.ltag ? first_cand(*fw_of(a, e), a.rtag0) : kNone;
        // elements after F: resolved here when F's mutation is absorbing (no RMWs: always; with RMWs: F's kind)
        uint16_t fkf = 0;
        if (TYPE == kLocal && a.fk && f != kNone && (uint32_t)i > f) fkf = a.fk[f];
        const bool after_abs = (uint32_t)i > f && f != kNone && (a.rounds == 0 || (fkf & 3u) == kFkWrite ||
                                                                  (fkf & 3u) == kFkReplay);
        if (f == kNone || (uint32_t)i < f || after_abs) {
            Meta m0 = m;
            if (after_abs) {
                if (a.rounds == 0) {
                    m0 = after_first<TYPE>(a, m, f, 0);
                } else {
                    int64_t fs;
                    batch_of(a, f, fs);
                    m0 = after_first_rmw(a, m, fkf, (uint8_t)(f - fs));
                }
            }
            Meta tm = m0;
            if (pd) dispatch<SV>(TYPE, xl, entry_of(a, e), idx, tm, c);
            else dispatch<SV>(TYPE, xg, entry_of(a, e), idx, tm, c);
            if (a.error_flags && !meta_equal(tm, m0)) atomicOr(a.error_flags, 1u);
        } else if ((uint32_t)i == f) {
            if (wave_shadow) cand = true;
            else apply_to_shadow<TYPE, SV>(a, nullptr, (uint32_t)i, entry_of(a, e));
            st = kStCommit;
        } else {
            a.pf[i] = f;
            st = kStPend;
        }
    }
    if (wave_shadow) apply_to_shadow_wave<TYPE, SV>(a, cand, (uint32_t)i, cand ? entry_of(a, e) : nullptr, vc, xl, pd);
    bool whole = false;   // a patched op whose every byte is known here: written whole by its lane
    if (pd) {
        uint8_t *cv = reinterpret_cast<uint8_t *>(cop) + kOpValueOff;
        if (vc.dst == cv) vc.dst = xg + kOpValueOff;
        if (vc.src == cv) {
            vc.src = fb ? nullptr : xg + kOpValueOff;
            vc.fill = fb ? 0x100u | fb : 0u;
        }
        whole = fb && vc.dst != xg + kOpValueOff;   // (a value the exec copies into the op replaces the fill)
    }
    if (SV != 31) wave_value_copies(vc, a.g.st_value, kVcBatch);
    if (kPir && a.hx) {
        // a whole op: key, header, flags, the value fill and the pad after it (launch_batch: at most 8 bytes,
        // in the op's last word), written by the wave, three ops a store instruction, so every 64-byte block
        // of the op is complete in L2 before it goes to HBM (whole ops stored by their own lane, 16 bytes
        // at a time: 4 % slower at configs[2])
        const uint32_t vend = kOpValueOff + a.g.st_value, w0 = (uint32_t)a.esz - 8u;
        const uint64_t pat = 0x0101010101010101ull * fb;
        const uint32_t nlow = vend - w0;
        const uint64_t lmask = nlow >= 8 ? ~0ull : (1ull << (8 * nlow)) - 1ull;
        wave_whole_ops(xg, whole, cop[0], cop[1], ((uint32_t)cop[2] & 0xFFFFu) | (fb << 16),
                       (pat & lmask) | (hw.b & ~lmask), (uint32_t)a.esz / 8u);
    }
    if (!in) return;
    a.st[i] = st;
    if (pd) {
        const uint64_t h0 = cop[0], h1 = cop[1], h2 = cop[2];
        const uint32_t vend = kOpValueOff + a.g.st_value, w0 = (uint32_t)a.esz - 8u;
        if (!whole) {   // the header from the copy, then the pad bytes after the value
            uint64_t *o = reinterpret_cast<uint64_t *>(xg);
            o[0] = h0;
            o[1] = h1;
            *reinterpret_cast<uint16_t *>(xg + 16) = (uint16_t)h2;
            if (vend < (uint32_t)a.esz) store_word_part(xg + w0, hw.b, vend - w0, 8u);
        }
        if (a.state_out) a.state_out[i] = (uint8_t)(h1 >> 8);
        return;
    }
    note_state(a, i, xg);
    // the op's first three and last 8-byte words stored again as they now stand, so that with the value a
    // GET copied the slab's lines are written whole (a line written with holes costs HBM a read-modify-write:
    // tools/write_bench.hip, 4M 312-byte ops with an 8-byte hole each 495 us against 241 us whole)
    if (SV != 31 && (a.esz & 7) == 0 && a.esz >= 32) {
        __threadfence_block();   // the wave's value copies before the loads
        uint64_t *o = reinterpret_cast<uint64_t *>(xg);
        const uint64_t h0 = o[0], h1 = o[1], h2 = o[2], t = o[a.esz / 8 - 1];
        o[0] = h0;
        o[1] = h1;
        o[2] = h2;
        o[a.esz / 8 - 1] = t;
    }
}

// Every other path: the patches go into the ops first (one thread per element), then the launch
// runs as usual
__global__ __launch_bounds__(256) void k_apply_patch(uint8_t *elems, const uint8_t *patch, int64_t n, int32_t esz,
                                                     uint32_t st_value)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const U64x2 p = *reinterpret_cast<const U64x2 *>(patch + i * 16);
    if (!patch_valid(p.b)) return;
    uint8_t *x = elems + i * esz;
    *reinterpret_cast<uint64_t *>(x) = p.a;
    x[8] = (uint8_t)p.b;
    x[9] = kNew;
    x[10] = (uint8_t)(p.b >> 8);
    if ((p.b >> 40) & 0xFFu) {
        x[11] = 0;
        *reinterpret_cast<uint32_t *>(x + 12) = 0;
    }
    *reinterpret_cast<uint16_t *>(x + 16) = (uint16_t)(p.b >> 16);
    const uint8_t fill = (uint8_t)(p.b >> 32);
    if (fill)
        for (uint32_t k = 0; k < st_value; ++k) x[kOpValueOff + k] = fill;
}

// ------------------------------------------------------------------ launches with unique keys
// HKV_BATCH_UNIQUE: no key appears twice among the launch's elements, so every element is its key's
// only one and sees S_0 in any serial order: after k_lookup's lookup (four lanes per element, two
// elements per lane group) lane 0 of the group runs the exec function on the element and the entry
// in place and stores the meta back -- one pass, each entry line read and written once. (INV
// launches: a peer's round slab, see hermeskv.h.) With check_unique every element also swaps its
// index into its key's F word, tagged with the launch; finding the launch's tag there means a
// second element of the key (error bit 4).
template <int TYPE, int SV>
__global__ __launch_bounds__(256) void k_unique(BatchArgs a)
{
    constexpr int P = 1;   // elements per lane group (launch_unique_t has the measurements)
    const int q = threadIdx.x & 3;
    const int gbase = (threadIdx.x & 63) & ~3;
    int64_t gi[P];
    uint64_t key[P], hdr[P];
    bool probe[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        gi[k] = ((int64_t)blockIdx.x * P + k) * 64 + (threadIdx.x >> 2);
        uint64_t kk = 0, hh = 0;
        bool p = false;
        if (gi[k] < a.n && q == 0) {
            int64_t start = 0;
            int32_t b = 0;
            bool in = true;
            if (a.offsets) {
                b = batch_of(a, gi[k], start);
            } else {
                b = (int32_t)(gi[k] / a.stride);
                start = (int64_t)b * a.stride;
                in = a.counts == nullptr || gi[k] - start < a.counts[b];
            }
            if (in) {
                const U64x2 h = *reinterpret_cast<const U64x2 *>(a.elems + gi[k] * a.esz);
                kk = h.a;
                hh = h.b;
                if (skip_elem_os(TYPE, (uint8_t)hh, (uint8_t)(hh >> 8))) {
                    if (TYPE == kInvs && a.ns_idx) atomicMax(&a.ns_idx[b], (int32_t)(gi[k] - start));
                } else {
                    p = true;
                }
            }
        }
        key[k] = (uint64_t)(uint32_t)__shfl((int)(uint32_t)kk, 0, 4) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(kk >> 32), 0, 4) << 32);
        probe[k] = __shfl((int)p, 0, 4) != 0;
        hdr[k] = hh;
    }
    bool ok[P];
    uint64_t phys[P];
    uint4 ln[P];
    lookup_pair<P>(a, key, probe, q, gbase, ok, phys, ln);
    Meta m[P];
    uint64_t ek[P];
#pragma unroll
    for (int k = 0; k < P; ++k) ek[k] = line_key_meta(ln[k], m[k]);
    if (q != 0) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (!probe[k]) continue;
        uint8_t *x = a.elems + gi[k] * a.esz;
        if (!(ok[k] && ek[k] == key[k])) {
            x[9] = kMiss;
            continue;
        }
        if (a.check_unique) {
            const unsigned long long v = ((unsigned long long)(~a.rtag0) << 32) | (uint32_t)gi[k];
            const unsigned long long old = atomicExch(a.fw + fw_index(a, phys[k]), v);
            if ((uint32_t)(old >> 32) == ~a.rtag0 && a.error_flags) atomicOr(a.error_flags, 16u);
        }
        uint8_t *entry = a.log + phys[k];
        Ctx c = make_ctx(a);
        uint8_t idx = 0;
        if (TYPE == kAcks) {   // the element's batch: its read_write_ops and their state mirror
            uint8_t *xx;
            elem_at(a, (uint32_t)gi[k], xx, idx, c);
        }
        Meta t = m[k];
        dispatch<SV>(TYPE, x, entry, idx, t, c);
        if (!meta_equal(t, m[k])) meta_store(entry, t);
    }
}

// k_unique for 64-B entries: the lookup as in k_local_fused (one wave per block, four lanes per
// element, each holding 16 B of the element and of the entry line), both staged in LDS, then one
// lane per element runs the exec function on the LDS copies; each lane writes back its 16-B chunks
// of the element and of the entry line that changed. The exec code touches LDS only, and the
// global writes are whole 16-B words.
__device__ __forceinline__ uint4 load_chunk(const uint8_t *x, int q, int32_t esz)
{
    if (16 * q + 16 <= esz) return *reinterpret_cast<const uint4 *>(x + 16 * q);
    if (16 * q + 8 <= esz) {
        const uint64_t t = *reinterpret_cast<const uint64_t *>(x + 16 * q);
        return make_uint4((uint32_t)t, (uint32_t)(t >> 32), 0u, 0u);
    }
    return make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ bool chunk_equal(const uint4 &a, const uint4 &b)
{
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

template <int TYPE, bool IL = false>
__global__ __launch_bounds__(64) void k_unique_lds(BatchArgs a)
{
    constexpr int P = 1;        // elements per lane group (launch_unique_t has the measurements)
    constexpr int E = 16 * P;   // elements per wave: P per lane group
    __shared__ uint4 sops[E * 4];
    __shared__ uint4 sln[E * 4];
    __shared__ uint32_t sent[E];
    __shared__ uint8_t sprb[E];
    const int tid = threadIdx.x, q = tid & 3, gbase = tid & ~3;
    const int64_t i0 = (int64_t)blockIdx.x * E;
    const int64_t n_live = a.offsets ? (int64_t)a.offsets[a.n_batches] : a.n;   // packed: past the last offset
    uint64_t key[P];
    bool probe[P], ok[P], live[P];
    uint64_t phys[P];
    uint4 ln[P], op[P];
    int te[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        te[k] = k * 16 + (tid >> 2);
        const int64_t i = i0 + te[k];
        live[k] = i < a.n && i < n_live;
        op[k] = live[k] ? load_chunk(a.elems + i * a.esz, q, a.esz) : make_uint4(0u, 0u, 0u, 0u);
        sops[te[k] * 4 + q] = op[k];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        key[k] = (uint64_t)(uint32_t)__shfl((int)op[k].x, 0, 4) | ((uint64_t)(uint32_t)__shfl((int)op[k].y, 0, 4) << 32);
        const uint32_t h0 = (uint32_t)__shfl((int)op[k].z, 0, 4);
        probe[k] = false;
        const int64_t i = i0 + te[k];
        if (live[k] && (a.offsets || in_count(a, (uint32_t)i))) {
            if (!skip_elem_os(TYPE, (uint8_t)h0, (uint8_t)(h0 >> 8))) {
                probe[k] = true;
            } else if (TYPE == kInvs && a.ns_idx && q == 0) {
                int64_t start;
                const int32_t b = batch_of(a, i, start);
                atomicMax(&a.ns_idx[b], (int32_t)(i - start));
            }
        }
    }
    uint8_t *home[P];   // (IL) where each hit's entry bytes live
    lookup_pair<P, IL>(a, key, probe, q, gbase, ok, phys, ln, home);
#pragma unroll
    for (int k = 0; k < P; ++k) {
        Meta m;
        const uint64_t ek = line_key_meta(ln[k], m);
        const bool hit = ok[k] && ek == key[k];
        sln[te[k] * 4 + q] = ln[k];
        if (q == 0) {
            sent[te[k]] = hit ? (uint32_t)(phys[k] / a.g.entry_unit) : kNone;
            sprb[te[k]] = probe[k];
        }
    }
    __syncthreads();
    if (tid < E && i0 + tid < n_live) {
        const int64_t i = i0 + tid;
        uint8_t *x = reinterpret_cast<uint8_t *>(&sops[tid * 4]);
        uint8_t *ent = reinterpret_cast<uint8_t *>(&sln[tid * 4]);
        const uint32_t e = sent[tid];
        if (e != kNone) {
            if (a.check_unique) {
                const unsigned long long v = ((unsigned long long)(~a.rtag0) << 32) | (uint32_t)i;
                const unsigned long long old = atomicExch(a.fw + fw_index(a, phys_of(a, e)), v);
                if ((uint32_t)(old >> 32) == ~a.rtag0 && a.error_flags) atomicOr(a.error_flags, 16u);
            }
            Ctx c = make_ctx(a);
            int done = -1;
            if (TYPE == kAcks) c.rw_done = &done;   // the batch is found only for a completion
            Meta m;
            meta_load(ent, m);
            Meta t = m;
            dispatch<31>(TYPE, x, ent, 0, t, c);
            if (!meta_equal(t, m)) meta_store(ent, t);
            if (TYPE == kAcks && done >= 0 && a.rw) {   // its read_write_ops slot and state mirror
                uint8_t *xx;
                uint8_t idx;
                elem_at(a, (uint32_t)i, xx, idx, c);
                complete_rw_slot(c, done);
            }
        } else if (sprb[tid]) {
            x[9] = kMiss;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (!live[k]) continue;
        uint4 w = sops[te[k] * 4 + q];
        if (TYPE == kInvs && a.ack_out) {
            // the ACK callbacks (ack_skip_or_get_sender_id, ack_copy_and_modify_elem,
            // ack_modify_elem_after_send; the k_marshal_acks of hkv_workload.hip) on the element as the
            // batch left it: the header chunk is lane 0's, the INV leaves as ST_EMPTY once answered
            uint8_t *y = a.ack_out + (i0 + te[k]) * a.ack_out_size;
            const uint32_t hz = sops[te[k] * 4].z;
            const uint8_t oc = (uint8_t)hz;
            const bool full = oc == kOpInvAbort && a.ack_out_size >= (uint32_t)a.esz;
            if (oc == kInvSuccess || full) {
                uint4 c = w;
                if (q == 0)
                    c.z = (hz & ~0xFFFFu) | (oc == kInvSuccess ? kOpAck : kOpInvAbort) |
                          ((uint32_t)(uint8_t)a.g.machine_id << 8);
                if (q == 0 || (full && 16 * q < a.esz)) {
                    if (16 * q + 16 <= a.esz || q == 0) *reinterpret_cast<uint4 *>(y + 16 * q) = c;
                    else *reinterpret_cast<uint64_t *>(y + 16 * q) = (uint64_t)c.x | ((uint64_t)c.y << 32);
                }
            } else if (q == 0) {
                y[8] = kEmpty;
            }
            if (q == 0 && (oc == kInvSuccess || oc == kOpInvAbort || oc == kOpMembChange))
                w.z = (w.z & ~0xFFu) | kEmpty;
        }
        if (!chunk_equal(w, op[k])) {
            uint8_t *xg = a.elems + (i0 + te[k]) * a.esz + 16 * q;
            if (16 * q + 16 <= a.esz) *reinterpret_cast<uint4 *>(xg) = w;
            else *reinterpret_cast<uint64_t *>(xg) = (uint64_t)w.x | ((uint64_t)w.y << 32);
        }
        if (ok[k] && q > 0) {   // bytes 0..15 of a log line (the MICA key) never change
            const uint4 l = sln[te[k] * 4 + q];
            if (!chunk_equal(l, ln[k])) reinterpret_cast<uint4 *>(IL ? home[k] : a.log + phys[k])[q] = l;
        }
    }
}

// HKV_BATCH_ROWS: k_unique_lds over positions instead of elements. Position j holds element j of
// every row, all of one key (or holes, opcode 0): the four lanes of a position load its element of
// every row and look the key up once, one lane applies the row elements in row order to the LDS copy
// of the entry -- exactly the rows' launches one after another, since each row holds the key once --
// and each element and the entry line are written back where they changed. An ACK's completion finds
// its read_write_ops once per position (the rows share the batch layout).
// No SGPR or occupancy attribute: 80 SGPRs and 8 waves per SIMD were within box noise.
//
// A packed ACK launch finds its positions' batches as the block's first loads, beside the element loads and the
// lookup, not after the resolve ("The ACK rows launch"): the wave narrows the offsets to a window
// around the block's first position (kary_last_le, two coalesced loads for up to 2^18 batches), keeps the
// window, one offset per lane twice, and every lane reads its own position's batch from it
// (rows_window_batch). A position past the window, after a long run of empty batches, asks batch_of as before.
// P: positions per lane group; 2, or 4 for a round's ACK launch at configs[1] (launch_rows).
template <int TYPE, int RMAX, int CH, int P = kLookupPair, bool IL = false>
__global__ __launch_bounds__(64) void k_unique_rows(BatchArgs a)
{
    constexpr int E = 16 * P;   // positions per wave: P per lane group
    // CH: 16-B chunks of an element held in LDS (1 for 16-B ACKs, 4 for 56-B INVs)
    __shared__ uint4 sops[RMAX][E * CH];
    __shared__ uint4 sln[E * 4];
    __shared__ uint32_t sent[E];
    __shared__ uint8_t spart[E];   // bit r: row r's element takes part (present, in count, not skipped)
    const int tid = threadIdx.x, q = tid & 3, gbase = tid & ~3;
    const int64_t i0 = (int64_t)blockIdx.x * E;
    const int R = a.n_rows < RMAX ? a.n_rows : RMAX;
    // packed rows may end before the stride: elements past the last batch offset are in no batch
    const int64_t n_live = a.offsets ? (int64_t)a.offsets[a.n_batches] : a.n;
    const auto is_live = [&](int64_t i) { return i < a.n && i < n_live && (a.offsets || in_count(a, (uint32_t)i)); };
    uint64_t key[P];
    bool probe[P], ok[P], live[P];
    uint64_t phys[P];
    // FLAT (the four-position instance, 16-B elements): lane t loads and writes back position t's element of
    // every row -- 4 VGPRs a row, not 4 for each of the lane group's positions -- and the lane groups read the
    // headers from LDS
    constexpr bool FLAT = P == 4 && CH == 1;
    const bool flat_live = FLAT && is_live(i0 + tid);
    uint4 ln[P], op[RMAX][FLAT ? 1 : P];
    uint32_t part[P];
    int te[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        te[k] = k * 16 + (tid >> 2);
        live[k] = is_live(i0 + te[k]);
    }
    if (FLAT) {
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const bool on = flat_live && r < R && r != a.skip_row;
            op[r][0] = on ? load_chunk(a.elems + (r * a.row_stride + i0 + tid) * a.esz, 0, a.esz) : make_uint4(0u, 0u, 0u, 0u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < (FLAT ? 1 : P); ++k) {
            const int64_t i = i0 + te[k];
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
                const bool on = live[k] && r < R && r != a.skip_row;
                op[r][k] = on && q < CH ? load_chunk(a.elems + (r * a.row_stride + i) * a.esz, q, a.esz)
                                        : make_uint4(0u, 0u, 0u, 0u);
            }
        }
    }
    // (packed ACK launches) the batch search's first step, in flight beside the elements; all of it is the wave's
    const bool locate = TYPE == kAcks && a.offsets && a.rw;
    int32_t blo = 0, bhi = a.n_batches - 1, bsample = 0;
    const auto sample = [&]() {   // this lane's sample of the step, INT32_MAX past the range
        const int32_t s = kary_sample(blo, bhi, tid);
        const int32_t v = a.offsets[s < bhi ? s : bhi];
        return s <= bhi ? v : INT32_MAX;
    };
    const auto narrow = [&]() { kary_narrow(blo, bhi, __popcll(__ballot((int64_t)bsample <= i0))); };
    const bool step1 = locate && bhi - blo >= kRowsWindow / 2;
    if (step1) bsample = sample();
    if (FLAT) {
#pragma unroll
        for (int r = 0; r < RMAX; ++r) sops[r][tid] = op[r][0];
        __syncthreads();
    } else {
#pragma unroll
        for (int k = 0; k < (FLAT ? 1 : P); ++k) {
#pragma unroll
            for (int r = 0; r < RMAX; ++r)
                if (q < CH) sops[r][te[k] * CH + q] = op[r][k];
        }
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        uint64_t kk = 0;
        uint32_t p = 0;
        bool mismatch = false;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            uint64_t kr;
            uint32_t h0;
            if (FLAT) {
                const uint4 h = sops[r][te[k]];
                kr = (uint64_t)h.x | ((uint64_t)h.y << 32);
                h0 = h.z;
            } else {
                const uint4 &h = op[r][FLAT ? 0 : k];
                kr = (uint64_t)(uint32_t)__shfl((int)h.x, 0, 4) | ((uint64_t)(uint32_t)__shfl((int)h.y, 0, 4) << 32);
                h0 = (uint32_t)__shfl((int)h.z, 0, 4);
            }
            if (!live[k] || r >= R || r == a.skip_row || (uint8_t)h0 == 0) continue;   // a hole
            if (skip_elem_os(TYPE, (uint8_t)h0, (uint8_t)(h0 >> 8))) continue;
            if (p && kr != kk) mismatch = true;
            if (!p) kk = kr;
            p |= 1u << r;
        }
        if (mismatch && q == 0 && a.error_flags) atomicOr(a.error_flags, 16u);
        key[k] = kk;
        part[k] = mismatch ? 0u : p;
        probe[k] = part[k] != 0;
    }
    uint8_t *home[P];   // (IL) where each hit's entry bytes live
    // the search's second step rides with the bucket loads, the window with the log lines
    bool step2 = false;
    lookup_pair_beside<P, IL>(a, key, probe, q, gbase, ok, phys, ln, home, [&]() {
        if (step1) narrow();
        step2 = locate && bhi - blo >= kRowsWindow / 2;
        if (step2) bsample = sample();
    });
    if (step2) narrow();
    while (locate && bhi - blo >= kRowsWindow / 2) {   // more than 2^18 batches
        bsample = sample();
        narrow();
    }
    // offsets blo .. blo + 127 (INT32_MAX where no batch is), two per lane
    int32_t w0 = INT32_MAX, w1 = INT32_MAX;
    if (locate) {
        if (blo + tid < a.n_batches) w0 = a.offsets[blo + tid];
        if (blo + 64 + tid < a.n_batches) w1 = a.offsets[blo + 64 + tid];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        Meta m;
        const uint64_t ek = line_key_meta(ln[k], m);
        const bool hit = ok[k] && ek == key[k];
        sln[te[k] * 4 + q] = ln[k];
        if (q == 0) {
            sent[te[k]] = hit ? (uint32_t)(phys[k] / a.g.entry_unit) : kNone;
            spart[te[k]] = (uint8_t)part[k];
        }
    }
    // lane t's position is i0 + t: its batch, or -1 (the window ended first, or there is nothing to locate)
    int32_t pb = -1;
    if (locate) {
        const int32_t k0 = __popcll(__ballot((int64_t)w0 <= i0)) - 1;   // the block's first batch, in the first 64
        const auto win = [&](int32_t j) { return __builtin_amdgcn_readlane(j < 64 ? w0 : w1, j & 63); };
        int32_t b;
        if (rows_window_batch(win, blo, k0 > 0 ? k0 : 0, i0 + tid, i0 + E - 1, b)) pb = b;
    }
    __syncthreads();
    if (tid < E && i0 + tid < n_live) {
        const int64_t i = i0 + tid;
        uint8_t *ent = reinterpret_cast<uint8_t *>(&sln[tid * 4]);
        const uint32_t e = sent[tid];
        const uint32_t p = spart[tid];
        if (e != kNone && p) {
            if (a.check_unique) {
                const unsigned long long v = ((unsigned long long)(~a.rtag0) << 32) | (uint32_t)i;
                const unsigned long long old = atomicExch(a.fw + fw_index(a, phys_of(a, e)), v);
                if ((uint32_t)(old >> 32) == ~a.rtag0 && a.error_flags) atomicOr(a.error_flags, 16u);
            }
            Ctx c = make_ctx(a);
            int done = -1;
            if (TYPE == kAcks) c.rw_done = &done;   // the batch is found only for a completion
            Meta m;
            meta_load(ent, m);
            Meta t = m;
#pragma unroll
            for (int r = 0; r < RMAX; ++r)
                if ((p >> r) & 1u) dispatch<31>(TYPE, reinterpret_cast<uint8_t *>(&sops[r][tid * CH]), ent, 0, t, c);
            if (!meta_equal(t, m)) meta_store(ent, t);
            if (TYPE == kAcks && done >= 0 && a.rw) {
                if (pb >= 0) {
                    batch_rw(a, pb, c);
                } else {
                    uint8_t *xx;
                    uint8_t idx;
                    elem_at(a, (uint32_t)i, xx, idx, c);
                }
                complete_rw_slot(c, done);
            }
        } else {
#pragma unroll
            for (int r = 0; r < RMAX; ++r)
                if ((p >> r) & 1u) reinterpret_cast<uint8_t *>(&sops[r][tid * CH])[9] = kMiss;
        }
    }
    __syncthreads();
    // chunk c of row r's element at position pos goes back where it differs from what was loaded (was)
    const auto put_back = [&](int r, int pos, int c, const uint4 &was) {
        uint4 w = sops[r][pos * CH + c];
        if (TYPE == kAcks && CH == 1 && a.ack_out) {
            // the VAL callbacks (hermes_worker.c:122-157, as shipped): an element whose opcode is not
            // ACK_SUCCESS, MEMBERSHIP_CHANGE or EMPTY is sent as a VAL from this machine, every
            // non-empty one leaves empty; a hole (opcode 0) is no element
            const uint8_t oc = (uint8_t)w.z;
            uint4 v = make_uint4(0u, 0u, (uint32_t)kEmpty, 0u);
            if (oc != 0 && oc != kAckSuccess && oc != kOpMembChange && oc != kEmpty)
                v = make_uint4(w.x, w.y, (w.z & ~0xFFFFu) | (uint32_t)kOpVal | ((uint32_t)(uint8_t)a.g.machine_id << 8), w.w);
            *reinterpret_cast<uint4 *>(a.ack_out + (r * a.row_stride + i0 + pos) * 16) = v;
            if (oc != 0 && oc != kEmpty) w.z = (w.z & ~0xFFu) | (uint32_t)kEmpty;
        }
        if (!chunk_equal(w, was)) {
            uint8_t *xg = a.elems + (r * a.row_stride + i0 + pos) * a.esz + 16 * c;
            if (16 * c + 16 <= a.esz) *reinterpret_cast<uint4 *>(xg) = w;
            else *reinterpret_cast<uint64_t *>(xg) = (uint64_t)w.x | ((uint64_t)w.y << 32);
        }
    };
    if (FLAT && flat_live) {
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
            if (r < R && r != a.skip_row) put_back(r, tid, 0, op[r][0]);
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (!live[k]) continue;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            if (FLAT || r >= R || r == a.skip_row || q >= CH) continue;
            put_back(r, te[k], q, op[r][FLAT ? 0 : k]);
        }
        if (ok[k] && q > 0) {   // bytes 0..15 of a log line (the MICA key) never change
            const uint4 l = sln[te[k] * 4 + q];
            if (!chunk_equal(l, ln[k])) reinterpret_cast<uint4 *>(IL ? home[k] : a.log + phys[k])[q] = l;
        }
    }
}

// k_unique for big objects (320-B entries, elements of up to 320 B: configs[2]): the same one pass,
// with each element and its whole entry staged in LDS by the element's four lanes (16-B chunks,
// coalesced), so the exec code -- 287-byte value copies included -- runs on LDS copies, and only the
// 16-B chunks that changed go back. One wave per kUbElems elements.
constexpr int kUbElems = 16;
constexpr int kUbChunks = 20;   // 320 B
template <int TYPE>
__global__ __launch_bounds__(64) void k_unique_big(BatchArgs a)
{
    // elements and entries in LDS; each lane keeps the chunks it loaded in registers (what changed goes
    // back), so a wave's LDS is 10 KB and four waves fit a SIMD
    __shared__ uint4 sx[kUbElems * kUbChunks];
    __shared__ uint4 se[kUbElems * kUbChunks];
    constexpr int kPerLane = (kUbChunks + 3) / 4;
    uint4 x0[kPerLane], e0[kPerLane];
    const int tid = threadIdx.x, q = tid & 3, el = tid >> 2, gbase = tid & ~3;
    const int64_t i = (int64_t)blockIdx.x * kUbElems + el;
    const bool live = i < a.n;
    const int nch = (a.esz + 15) / 16;
    uint8_t *xg = a.elems + i * a.esz;
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) {
        const int c = q + 4 * u;
        const uint4 v = live && c < nch ? load_chunk(xg, c, a.esz) : make_uint4(0u, 0u, 0u, 0u);
        if (c < nch) sx[el * kUbChunks + c] = v;
        x0[u] = v;
    }
    const uint4 c0 = sx[el * kUbChunks];   // the element's key and header (every lane of the group)
    const uint64_t key = (uint64_t)c0.x | ((uint64_t)c0.y << 32);
    bool probe = false;
    if (live && (a.offsets || in_count(a, (uint32_t)i))) {
        if (!skip_elem_os(TYPE, (uint8_t)c0.z, (uint8_t)(c0.z >> 8))) {
            probe = true;
        } else if (TYPE == kInvs && a.ns_idx && q == 0) {
            int64_t start;
            const int32_t b = batch_of(a, i, start);
            atomicMax(&a.ns_idx[b], (int32_t)(i - start));
        }
    }
    bool ok;
    uint64_t phys;
    uint4 ln;
    lookup_pair<1>(a, &key, &probe, q, gbase, &ok, &phys, &ln);
    Meta m0;
    const uint64_t ek = line_key_meta(ln, m0);
    const bool hit = ok && ek == key;
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) e0[u] = make_uint4(0u, 0u, 0u, 0u);
    if (hit) {
        const uint4 *eg = reinterpret_cast<const uint4 *>(a.log + phys);
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            const int c = q + 4 * u;
            if (c >= kUbChunks) continue;
            const uint4 v = c < 4 ? ln : eg[c];
            se[el * kUbChunks + c] = v;
            e0[u] = v;
        }
    }
    __syncthreads();
    if (q == 0 && live) {
        uint8_t *x = reinterpret_cast<uint8_t *>(&sx[el * kUbChunks]);
        uint8_t *ent = reinterpret_cast<uint8_t *>(&se[el * kUbChunks]);
        if (hit) {
            if (a.check_unique) {
                const unsigned long long v = ((unsigned long long)(~a.rtag0) << 32) | (uint32_t)i;
                const unsigned long long old = atomicExch(a.fw + fw_index(a, phys), v);
                if ((uint32_t)(old >> 32) == ~a.rtag0 && a.error_flags) atomicOr(a.error_flags, 16u);
            }
            Ctx c = make_ctx(a);
            int done = -1;
            if (TYPE == kAcks) c.rw_done = &done;   // the batch is found only for a completion
            Meta m;
            meta_load(ent, m);
            Meta t = m;
            dispatch<287>(TYPE, x, ent, 0, t, c);
            if (!meta_equal(t, m)) meta_store(ent, t);
            if (TYPE == kAcks && done >= 0 && a.rw) {   // its read_write_ops slot and state mirror
                uint8_t *xx;
                uint8_t idx;
                elem_at(a, (uint32_t)i, xx, idx, c);
                complete_rw_slot(c, done);
            }
        } else if (probe) {
            x[9] = kMiss;
        }
    }
    __syncthreads();
    if (live) {
        const uint32_t hz = sx[el * kUbChunks].z;   // the element's opcode after the batch (byte 8)
        const uint8_t oc = (uint8_t)hz;
        if (TYPE == kInvs && a.ack_out) {
            // the ACK callbacks on the element as the batch left it (as in k_unique_lds): an INV_SUCCESS
            // answers with its header, an OP_INV_ABORT with the whole element when the ACK slot holds it
            uint8_t *y = a.ack_out + i * a.ack_out_size;
            const bool full = oc == kOpInvAbort && a.ack_out_size >= (uint32_t)a.esz;
            if (oc == kInvSuccess || full) {
                for (int c = q; c < (full ? nch : 1); c += 4) {
                    uint4 w = sx[el * kUbChunks + c];
                    if (c == 0)
                        w.z = (hz & ~0xFFFFu) | (oc == kInvSuccess ? kOpAck : kOpInvAbort) |
                              ((uint32_t)(uint8_t)a.g.machine_id << 8);
                    if (16 * c + 16 <= a.esz || c == 0) *reinterpret_cast<uint4 *>(y + 16 * c) = w;
                    else *reinterpret_cast<uint64_t *>(y + 16 * c) = (uint64_t)w.x | ((uint64_t)w.y << 32);
                }
            } else if (q == 0) {
                y[8] = kEmpty;
            }
        }
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            const int c = q + 4 * u;
            if (c >= nch) continue;
            uint4 w = sx[el * kUbChunks + c];
            if (TYPE == kInvs && a.ack_out && c == 0 && (oc == kInvSuccess || oc == kOpInvAbort || oc == kOpMembChange))
                w.z = (w.z & ~0xFFu) | kEmpty;   // answered (ack_modify_elem_after_send)
            if (chunk_equal(w, x0[u])) continue;
            if (16 * c + 16 <= a.esz) *reinterpret_cast<uint4 *>(xg + 16 * c) = w;
            else *reinterpret_cast<uint64_t *>(xg + 16 * c) = (uint64_t)w.x | ((uint64_t)w.y << 32);
        }
    }
    if (hit) {   // bytes 0..15 of an entry (the MICA key) never change
        uint4 *eg = reinterpret_cast<uint4 *>(a.log + phys);
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            const int c = q + 4 * u;
            if (c >= kUbChunks) continue;
            const uint4 w = se[el * kUbChunks + c];
            if (c > 0 && !chunk_equal(w, e0[u])) eg[c] = w;
        }
    }
}

// Round r >= 1 resolve over the pending elements (sparse: direct global access), against S_r in
// the shadow of round r-1's first candidate of the element's key.
// After the last round, elements still pending go to the fallback list.
template <int TYPE, int SV>
__global__ __launch_bounds__(256) void k_resolve(BatchArgs a, int r)
{
    // 16-B messages (ACKs, VALs): the element is dispatched on an LDS copy, one 16-B access in and
    // one out instead of the exec functions' byte-wise global accesses. (A 56-B op costs more to
    // write back whole than the one or two bytes an INV changes.)
    extern __shared__ uint64_t sx[];
    const bool kStage = SV == 31 && a.esz <= 16;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool left = false;
    // big values: copied a wave per value after the exec calls (see k_resolve0_direct); the shadow
    // they read (round r-1's first candidate's) is not written in this round
    VCopy vc{nullptr, nullptr};
    VCopy *vcp = SV != 31 && a.g.st_value <= 320 ? &vc : nullptr;
    const bool wave_shadow = SV != 31 && vcp;   // see k_resolve0_direct
    bool cand = false;
    uint32_t prev = 0;
    if (i < a.n && a.st[i] == kStPend) {
        const uint32_t e = a.ent[i];
        const uint32_t f = first_cand(*fw_of(a, e), a.rtag0 + (uint32_t)r);
        prev = a.pf[i];  // S_r lives in the shadow of round r-1's first candidate
        if (f == kNone || (uint32_t)i <= f) {
            uint8_t *xg = a.elems + i * a.esz;
            uint8_t *xl = reinterpret_cast<uint8_t *>(sx) + threadIdx.x * (uint32_t)a.esz;
            if (kStage) copy_elem(xl, xg, a.esz);
            if ((uint32_t)i != f) {
                if (kStage) resolve_elem<TYPE, SV>(a, (uint32_t)i, xl, shadow_of(a, prev));
                else resolve_elem<TYPE, SV>(a, (uint32_t)i, xg, shadow_of(a, prev), vcp);
                a.st[i] = kStDone;
            } else {
                if (wave_shadow) cand = true;
                else apply_to_shadow<TYPE, SV>(a, kStage ? xl : nullptr, (uint32_t)i, shadow_of(a, prev));
                a.st[prev] = kStDone;  // superseded
                a.st[i] = kStCommit;
            }
            if (kStage) copy_elem(xg, xl, a.esz);
            if (!cand) note_state(a, i, kStage ? xl : xg);
        } else {
            a.pf[i] = f;  // after the last round: identifies the key's run in k_fb_exec
            left = r == a.rounds;
        }
    }
    if (wave_shadow) {
        apply_to_shadow_wave<TYPE, SV>(a, cand, (uint32_t)i, cand ? shadow_of(a, prev) : nullptr, vc);
        if (cand) note_state(a, i, a.elems + i * a.esz);
    }
    if (SV != 31) wave_value_copies(vc, a.g.st_value, kVcBatch);
    if (r == a.rounds) {  // wave-aggregated append (uniform branch)
        const uint32_t t = agg_ticket(&a.ctr[kCtrFbL], 0u, left);
        if (left) a.fbl[t] = (uint32_t)i;
    }
}

// ------------------------------------------------------------------ fallback
__device__ __forceinline__ uint32_t pow2ceil(uint32_t c) { return c <= 1 ? 1u : 1u << (32 - __clz(c - 1)); }

// Final commit of a launch: every key's last shadow becomes its entry.
template <int SV>
__global__ __launch_bounds__(256) void k_commit(BatchArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (SV != 31) {  // big entries: copied by the whole wave, 16 B per lane, several entries per step
        const bool mine = i < a.n && a.st[i] == kStCommit;
        const uint32_t e = mine ? a.ent[i] : 0u;
        wave_block_copies(mine ? entry_of(a, e) : nullptr, mine ? shadow_of(a, (uint32_t)i) : nullptr,
                          a.g.entry_size);
        return;
    }
    if (i >= a.n || a.st[i] != kStCommit) return;
    uint8_t *dst = entry_of(a, a.ent[i]);
    const uint8_t *src = shadow_of(a, (uint32_t)i);
    if (SV == 31) {  // 64-B entries and shadows are 16-byte aligned
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        const uint4 w0 = s4[0], w1 = s4[1], w2 = s4[2], w3 = s4[3];
        d4[0] = w0;
        d4[1] = w1;
        d4[2] = w2;
        d4[3] = w3;
    } else {
        copy_entry(dst, src, a.g.entry_size);
    }
}

constexpr int kFbThreads = 1024;
constexpr int kFbPerThread = 8;
constexpr int kFbChunk = kFbThreads * kFbPerThread;
constexpr int kFbLds = 8192;    // (F_R, element) pairs sorted in LDS
constexpr int kFbSerial = 32;   // runs up to this long are applied by one thread

__device__ __forceinline__ int block_min(int v, int *lds)
{
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = lds[0];
#pragma unroll
    for (int w = 1; w < kFbThreads / 64; ++w) r = lds[w] < r ? lds[w] : r;
    return r;
}

// ascending bitonic sort of n (a power of two) words, by the whole workgroup
__device__ void bitonic_sort(unsigned long long *s, uint32_t n)
{
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
                const uint32_t u = t ^ j;
                if (u > t) {
                    const unsigned long long x = s[t], y = s[u];
                    if ((x > y) == ((t & k) == 0)) {
                        s[t] = y;
                        s[u] = x;
                    }
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

// Elements still pending after the last round (the fallback list), after k_commit: every such
// element's key had a first candidate F_R in the last round, whose index it holds in pf. Workgroup
// b owns the keys with F_R % gridDim == b: it gathers their members as (F_R, element) pairs (LDS,
// or a region of mem beyond kFbLds pairs), sorts them (each key is then one run in element order)
// and finishes each run from the committed entry with first-candidate passes: repeat {block min
// of the first candidate f against the shared meta; resolve members before f on private copies;
// barrier; f applies; barrier} over chunks of kFbChunk members until a chunk has no candidate.
template <int TYPE, int SV>
__global__ __launch_bounds__(kFbThreads) void k_fb_exec(BatchArgs a)
{
    __shared__ unsigned long long srt[kFbLds];
    __shared__ Meta sm;
    __shared__ int red[kFbThreads / 64];
    __shared__ uint32_t lcnt, loff;
    const int tid = threadIdx.x;
    const uint32_t nl = a.ctr[kCtrFbL];
    if (nl == 0) return;  // uniform
    const uint32_t G = gridDim.x, me = blockIdx.x;
    if (tid == 0) lcnt = 0;
    __syncthreads();
    for (uint32_t j = tid; j < nl; j += kFbThreads)
        if (a.pf[a.fbl[j]] % G == me) atomicAdd(&lcnt, 1u);
    __syncthreads();
    const uint32_t cnt = lcnt, p2 = pow2ceil(cnt);
    if (cnt == 0) return;  // uniform
    unsigned long long *ord = srt;
    if (p2 > (uint32_t)kFbLds) {
        if (tid == 0) loff = atomicAdd(&a.ctr[kCtrFbM], p2);
        __syncthreads();
        ord = a.mem + loff;
    }
    __syncthreads();
    if (tid == 0) lcnt = 0;
    __syncthreads();
    for (uint32_t j = tid; j < nl; j += kFbThreads) {
        const uint32_t i = a.fbl[j], f = a.pf[i];
        if (f % G == me) ord[atomicAdd(&lcnt, 1u)] = ((unsigned long long)f << 32) | i;
    }
    for (uint32_t j = cnt + tid; j < p2; j += kFbThreads) ord[j] = ~0ull;
    __threadfence_block();
    __syncthreads();
    bitonic_sort(ord, p2);
    Ctx c = make_ctx(a);
    // serial tier: the head of a run of at most kFbSerial members applies it alone, in order
    for (uint32_t p = tid; p < cnt; p += kFbThreads) {
        const uint32_t kf = (uint32_t)(ord[p] >> 32);
        if (p > 0 && (uint32_t)(ord[p - 1] >> 32) == kf) continue;
        uint32_t re = p + 1;
        while (re < cnt && re - p <= (uint32_t)kFbSerial && (uint32_t)(ord[re] >> 32) == kf) ++re;
        if (re - p > (uint32_t)kFbSerial) continue;
        uint8_t *entry = entry_of(a, a.ent[(uint32_t)ord[p]]);
        Meta m;
        meta_load(entry, m);
        for (uint32_t q = p; q < re; ++q) {
            uint8_t *x;
            uint8_t idx;
            elem_at(a, (uint32_t)ord[q], x, idx, c);
            dispatch<SV>(TYPE, x, entry, idx, m, c);
            note_state(a, (uint32_t)ord[q], x);
        }
        meta_store(entry, m);
    }
    __syncthreads();
    for (uint32_t rs = 0; rs < cnt;) {  // longer runs: one at a time, by the whole workgroup
        const uint32_t key_f = (uint32_t)(ord[rs] >> 32);
        if (tid == 0) {
            uint32_t re = rs + 1;
            while (re < cnt && (uint32_t)(ord[re] >> 32) == key_f) ++re;
            loff = re;
            if (re - rs > (uint32_t)kFbSerial) meta_load(entry_of(a, a.ent[(uint32_t)ord[rs]]), sm);
        }
        __threadfence_block();
        __syncthreads();
        const uint32_t re = loff;
        if (re - rs <= (uint32_t)kFbSerial) {  // uniform: done by the serial tier
            __syncthreads();
            rs = re;
            continue;
        }
        uint8_t *entry = entry_of(a, a.ent[(uint32_t)ord[rs]]);
        for (uint32_t base = rs; base < re; base += kFbChunk) {
            uint32_t pending = 0;
#pragma unroll
            for (int j = 0; j < kFbPerThread; ++j)
                if (base + j * kFbThreads + tid < re) pending |= 1u << j;
            for (;;) {
                const Meta m = sm;
                int mine = kFbChunk;
#pragma unroll
                for (int j = kFbPerThread - 1; j >= 0; --j) {
                    if (!(pending >> j & 1u)) continue;
                    uint8_t *x;
                    uint8_t idx;
                    elem_at(a, (uint32_t)ord[base + j * kFbThreads + tid], x, idx, c);
                    if (would_mutate(TYPE, x, m, c)) mine = j * kFbThreads + tid;
                }
                const int f = block_min(mine, red);
#pragma unroll
                for (int j = 0; j < kFbPerThread; ++j) {
                    const int pos = j * kFbThreads + tid;
                    if (!(pending >> j & 1u) || pos >= f) continue;
                    uint8_t *x;
                    uint8_t idx;
                    elem_at(a, (uint32_t)ord[base + pos], x, idx, c);
                    Meta t = m;
                    dispatch<SV>(TYPE, x, entry, idx, t, c);
                    if (a.error_flags && !meta_equal(t, m)) atomicOr(a.error_flags, 1u);
                    note_state(a, (uint32_t)ord[base + pos], x);
                    pending &= ~(1u << j);
                }
                __syncthreads();  // every read of the entry value precedes the mutation
                if (f < kFbChunk && (f % kFbThreads) == tid) {
                    uint8_t *x;
                    uint8_t idx;
                    elem_at(a, (uint32_t)ord[base + f], x, idx, c);
                    Meta mm = m;
                    dispatch<SV>(TYPE, x, entry, idx, mm, c);
                    note_state(a, (uint32_t)ord[base + f], x);
                    pending &= ~(1u << (f / kFbThreads));
                    sm = mm;
                }
                __threadfence_block();
                __syncthreads();
                if (f >= kFbChunk) break;
            }
        }
        if (tid == 0) meta_store(entry, sm);
        __threadfence_block();
        __syncthreads();
        rs = re;
    }
}

// ------------------------------------------------------------------ partitioned host launches
// The combining submit's launches on 64-B entries (HostPartLaunch, hkv_internal.h). Workgroup g
// takes partition g of every batch: all elements of its keys, in element order, and no other
// workgroup's. So the k_small rounds run per workgroup with no communication at all, and a
// launch's latency stays that of one partition however many callers it combines:
//   load    its slice of each batch straight from the callers' pinned buffers into LDS (one
//           thread per element, four 16-B loads), with each element's position in its batch
//   lookup  one thread per element (hermesKV.c:938-993): bucket, tag probe, wrap, the whole
//           64-B entry line into LDS; the elements of one entry share the copy of its first one
//   rounds  k_small's element-order rounds on the LDS copies (candidates lower their key's F,
//           elements before F resolve on private metas, F applies to the shared copy); after
//           kHpRounds the first pending element of a key finishes it serially
//   store   changed entry lines back to HBM (the 48 bytes after the MICA key), every element back
//           to its caller's buffer with system-scope stores, then flags[g] = seq
// A completing ACK marks its read_write_ops slot in the caller's pinned copy directly (one byte,
// system scope); node_suspected is the host's (hermes_skip_inv depends on the element alone).
constexpr int kHpThreads = kPartCap;          // one element per thread
constexpr int kHpSlots = 2 * kPartCap;        // entry-id hash slots
constexpr int kHpRounds = 8;
constexpr int kHpWords = kPartCap * 8 / kHpThreads;   // 8-byte words of elements per thread (esz <= 64)

__device__ __forceinline__ uint32_t hp_slot(uint32_t *hkey, uint32_t e)
{
    uint32_t h = (e * 0x9E3779B1u) >> (32 - 9);   // kHpSlots = 2^9
    for (;;) {
        const uint32_t old = atomicCAS(&hkey[h], kNone, e);
        if (old == kNone || old == e) return h;
        h = (h + 1) & (kHpSlots - 1);
    }
}

// Host memory the callers rewrite between launches is read with system-scope (uncached) loads: the
// serving kernel (k_hserve) outlives many launches, so no kernel start invalidates stale lines for it.
__device__ __forceinline__ uint64_t ld_sys64(const void *p)
{
    return __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint32_t ld_sys32(const void *p)
{
    return __hip_atomic_load(reinterpret_cast<const uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint32_t ld_sys_u16(const uint16_t *p)   // 2-byte aligned
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return (ld_sys32(reinterpret_cast<const void *>(a & ~(uintptr_t)3)) >> (8 * (a & 2))) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t ld_sys_u8(const uint8_t *p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return (ld_sys32(reinterpret_cast<const void *>(a & ~(uintptr_t)3)) >> (8 * (a & 3))) & 0xFFu;
}

// exec_ack's read_write_ops completion of slot `done` in a caller's pinned copy (hermesKV.c:660-668).
// pre: bytes 8..11 of slot pre_slot, read ahead (hp_rw_ahead); a slot of another opcode keeps its state,
// so it is not written at all.
__device__ __forceinline__ void hp_complete_rw(uint8_t *rw, int done, uint32_t op_size, uint32_t pre = 0, int pre_slot = -1)
{
    uint8_t *w = rw + (size_t)done * op_size;
    const uint8_t oc = done == pre_slot ? (uint8_t)pre : (uint8_t)ld_sys_u8(w + 8);
    if (oc != kOpGet && oc != kOpPut && oc != kOpRmw) return;
    const uint8_t ns = oc == kOpGet ? kNew : oc == kOpPut ? kPutComplete : kRmwComplete;
    __hip_atomic_store(w + 9, ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// An ACK's read_write_ops slot is the entry's op-buffer index (exec_ack): its opcode is read right after
// the lookup, so the read overlaps the rounds instead of following them -- from the opcodes the caller
// staged in device memory (rwo), else from byte 8 of the slot in the pinned copy (over PCIe)
__device__ __forceinline__ void hp_rw_ahead(const uint8_t *rw, const uint8_t *rwo, const uint8_t *line, uint32_t op_size,
                                            uint32_t &pre, int &pre_slot)
{
    Meta m;
    meta_load(line, m);
    const int ob = m_obi(m);
    if (ob == kObiEmpty) return;
    pre = rwo ? ld_sys_u8(rwo + ob) : ld_sys_u8(rw + (size_t)ob * op_size + 8);
    pre_slot = ob;
}

// The LDS of one partition's work (both kernels)
struct HpLds {
    uint4 sel[kPartCap * 4];        // elements (64 B per slot, esz used)
    uint4 sln[kPartCap * 4];        // entry lines; a key's elements use its first slot's
    HostPartHdr bh[kPartMaxB];
    int32_t base[kPartMaxB + 1], lo[kPartMaxB], wbase[kPartMaxB + 1];
    uint16_t prow[2][kPartMaxB];    // part[g][*], part[g + 1][*]
    uint32_t hkey[kHpSlots], hmin[kHpSlots], hf[kHpSlots];
    uint8_t sdirty[kPartCap], spend[kPartCap];
    uint16_t shs[kPartCap];
    int cmd;
    int32_t nb;
    int32_t nm;                     // k_hserve: launches taken in this pass
    int32_t sb[kPartMaxB + 1];      // ... their first batches (sb[nm]: all of them)
};

// The batch ranges of partition g (bh, prow in LDS): per-batch slot and word offsets (one wave)
__device__ __forceinline__ void hp_scan(HpLds &L, int nb)
{
    const int tid = threadIdx.x;
    if (tid < 64) {
        int32_t c = 0, cw = 0;
        if (tid < nb) {
            const int32_t a0 = L.prow[0][tid], a1 = L.prow[1][tid];
            L.lo[tid] = a0;
            c = a1 - a0;
            cw = c * (L.bh[tid].esz / 8);
        }
        int32_t incl = c, inclw = cw;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t v = __shfl_up(incl, d, 64), vw = __shfl_up(inclw, d, 64);
            if (tid >= d) {
                incl += v;
                inclw += vw;
            }
        }
        if (tid < nb) {
            L.base[tid + 1] = incl;
            L.wbase[tid + 1] = inclw;
        }
        if (tid == 0) {
            L.base[0] = 0;
            L.wbase[0] = 0;
        }
    }
}

__device__ __forceinline__ int hp_batch_of(const int32_t *offs, int nb, int v)   // the last b with offs[b] <= v
{
    int l = 0, h = nb;
    while (h - l > 1) {
        const int mid = (l + h) >> 1;
        if (offs[mid] <= v) l = mid;
        else h = mid;
    }
    return l;
}

// Partition g of one launch whose headers and ranges are in L (after hp_scan and a barrier):
// load, lookup, rounds, store back, then flags[g] = seq. See the section comment.
__device__ void hp_partition(const HostPartCommon &p, HpLds &L, int g, int nb, uint32_t seq)
{
    const int tid = threadIdx.x;
    const bool pr = p.prof && g == 0 && tid == 0;
    if (pr) p.prof[1] = wall_clock64();
    for (int j = tid; j < kHpSlots; j += kHpThreads) {
        L.hkey[j] = kNone;
        L.hmin[j] = kNone;
        L.hf[j] = kNone;
    }
    const int P = L.base[nb];   // at most kPartCap (the host's check)
    const int s = tid;
    const bool live = s < P;
    const int b = live ? hp_batch_of(L.base, nb, s) : 0;
    const HostPartHdr &hd = L.bh[b];
    const int64_t j = live ? (int64_t)L.lo[b] + (s - L.base[b]) : 0;
    // the elements: each batch's slice is contiguous in its caller's buffer, so consecutive lanes
    // copy consecutive 8-byte words of it (coalesced requests over PCIe), all loads in flight at once
    const uint16_t pos = live ? (uint16_t)ld_sys_u16(reinterpret_cast<const uint16_t *>(hd.pos) + j) : (uint16_t)0;
    {
        const int TW = L.wbase[nb];   // at most kPartCap * 8
        uint64_t w[kHpWords];
        int dst[kHpWords];
#pragma unroll
        for (int r = 0; r < kHpWords; ++r) {
            const int idx = tid + r * kHpThreads;
            dst[r] = -1;
            w[r] = 0;
            if (idx < TW) {
                const int l = hp_batch_of(L.wbase, nb, idx);
                const int per = L.bh[l].esz / 8, wi = idx - L.wbase[l];
                w[r] = ld_sys64(reinterpret_cast<const uint8_t *>(L.bh[l].elems) + ((int64_t)L.lo[l] * L.bh[l].esz + 8 * wi));
                dst[r] = (L.base[l] + wi / per) * 8 + wi % per;
            }
        }
#pragma unroll
        for (int r = 0; r < kHpWords; ++r)
            if (dst[r] >= 0) reinterpret_cast<uint64_t *>(L.sel)[dst[r]] = w[r];
    }
    __syncthreads();
    uint8_t *x = reinterpret_cast<uint8_t *>(&L.sel[s * 4]);
    Ctx c;
    c.g = p.g;
    c.g_membership = hd.g_membership;
    c.w_ack_init = hd.w_ack_init;
    c.rw = reinterpret_cast<uint8_t *>(hd.rw);
    c.rws = nullptr;
    c.rw_done = nullptr;
    c.vc = nullptr;
    const int type = hd.type;
    // lookup (hermesKV.c:938-993)
    uint32_t e = kNone;
    uint64_t phys = 0;
    if (live && !skip_elem_os(type, x[8], x[9])) {
        const uint64_t key = *reinterpret_cast<const uint64_t *>(x);
        const uint4 *bk = bucket_words(p.index, bucket_of(p.g, key));
        const uint4 q0 = bk[0], q1 = bk[1], q2 = bk[2], q3 = bk[3];
        const uint64_t sl[8] = {u64_of(q0.x, q0.y), u64_of(q0.z, q0.w), u64_of(q1.x, q1.y), u64_of(q1.z, q1.w),
                                u64_of(q2.x, q2.y), u64_of(q2.z, q2.w), u64_of(q3.x, q3.y), u64_of(q3.z, q3.w)};
        const uint32_t tag = key_tag(key);
        int hit = -1;
#pragma unroll
        for (int q = 7; q >= 0; --q)
            if (slot_matches(sl[q], tag)) hit = q;
        if (hit >= 0) {
            const uint64_t off = slot_off_raw(sl[hit]);
            if (in_log_window(p.g, off)) {
                phys = off & p.g.log_mask;
                const uint4 *ln = reinterpret_cast<const uint4 *>(p.log + phys);
                const uint4 l0 = ln[0], l1 = ln[1], l2 = ln[2], l3 = ln[3];
                if (u64_of(l0.z, l0.w) == key) {
                    e = (uint32_t)(phys / p.g.entry_unit);
                    L.sln[s * 4 + 0] = l0;
                    L.sln[s * 4 + 1] = l1;
                    L.sln[s * 4 + 2] = l2;
                    L.sln[s * 4 + 3] = l3;
                }
            }
        }
        if (e == kNone) x[9] = kMiss;
    }
    uint32_t rw_pre = 0;
    int rw_pre_slot = -1;
    if (type == kAcks && hd.rw && e != kNone)
        hp_rw_ahead(reinterpret_cast<const uint8_t *>(hd.rw), reinterpret_cast<const uint8_t *>(hd.rwo),
                    reinterpret_cast<const uint8_t *>(&L.sln[s * 4]), p.g.op_size, rw_pre, rw_pre_slot);
    if (pr) p.prof[2] = wall_clock64();
    uint32_t hs = 0;
    if (e != kNone) {
        hs = hp_slot(L.hkey, e);
        atomicMin(&L.hmin[hs], (uint32_t)s);
    }
    __syncthreads();
    const int cs = e != kNone ? (int)L.hmin[hs] : s;   // the slot whose line copy the key's elements share
    uint8_t *ent = reinterpret_cast<uint8_t *>(&L.sln[cs * 4]);
    const uint8_t idx = (uint8_t)pos;
    bool pend = e != kNone, dirty = false;
    int done = -1;
    c.rw_done = type == kAcks ? &done : nullptr;
    bool any = true;
    for (int r = 0;; ++r) {
        any = __syncthreads_or(pend);
        if (!any || r == kHpRounds) break;
        Meta m;
        if (pend) {
            meta_load(ent, m);
            if (would_mutate(type, x, m, c)) atomicMin(&L.hf[hs], (uint32_t)s);
        }
        __syncthreads();
        if (pend && L.hf[hs] > (uint32_t)s) {   // before the key's candidate: S_r, unchanged
            Meta t = m;
            dispatch<31>(type, x, ent, idx, t, c);
            if (p.error_flags && !meta_equal(t, m)) atomicOr(p.error_flags, 1u);
            pend = false;
        }
        __syncthreads();   // every read of S_r precedes the mutation
        if (pend && L.hf[hs] == (uint32_t)s) {  // the candidate: S_r -> S_{r+1}
            dispatch<31>(type, x, ent, idx, m, c);
            meta_store(ent, m);
            L.hf[hs] = kNone;
            dirty = true;
            pend = false;
        }
    }
    if (any) {  // keys that kept mutating: each key's first pending element finishes it in order
        L.spend[s] = pend;
        L.shs[s] = (uint16_t)hs;
        __syncthreads();   // (every F of the last round was reset to kNone when it applied)
        if (pend) atomicMin(&L.hf[hs], (uint32_t)s);
        __syncthreads();
        if (pend && L.hf[hs] == (uint32_t)s) {
            Meta m;
            meta_load(ent, m);
            for (int k = s; k < P; ++k) {
                if (!L.spend[k] || L.shs[k] != (uint16_t)hs) continue;   // hash slot = entry = key
                uint8_t *xk = reinterpret_cast<uint8_t *>(&L.sel[k * 4]);
                Ctx ck = c;
                int dk = -1;
                ck.rw_done = type == kAcks ? &dk : nullptr;
                const int l = hp_batch_of(L.base, nb, k);   // the element's own batch
                ck.g_membership = L.bh[l].g_membership;
                ck.w_ack_init = L.bh[l].w_ack_init;
                ck.rw = reinterpret_cast<uint8_t *>(L.bh[l].rw);
                const int64_t jk = (int64_t)L.lo[l] + (k - L.base[l]);
                const uint8_t ik = (uint8_t)ld_sys_u16(reinterpret_cast<const uint16_t *>(L.bh[l].pos) + jk);
                dispatch<31>(L.bh[l].type, xk, ent, ik, m, ck);
                if (dk >= 0 && ck.rw) hp_complete_rw(ck.rw, dk, p.g.op_size);
            }
            meta_store(ent, m);
            dirty = true;
        }
    }
    // a completing ACK of the rounds marks its read_write_ops slot (exec_ack left it to us)
    if (done >= 0 && c.rw) hp_complete_rw(c.rw, done, p.g.op_size, rw_pre, rw_pre_slot);
    if (pr) p.prof[3] = wall_clock64();
    L.sdirty[s] = 0;
    __syncthreads();
    if (dirty) L.sdirty[cs] = 1;
    __syncthreads();
    // the changed entry lines back to HBM (bytes 16..63: the MICA key never changes)
    if (live && e != kNone && cs == s && L.sdirty[s]) {
        uint4 *dst = reinterpret_cast<uint4 *>(p.log + phys);
        dst[1] = L.sln[s * 4 + 1];
        dst[2] = L.sln[s * 4 + 2];
        dst[3] = L.sln[s * 4 + 3];
    }
    // every element back to its caller (consecutive lanes, consecutive words), then the flag (see
    // k_small's copy-out)
    for (int w = tid; w < L.wbase[nb]; w += kHpThreads) {
        const int l = hp_batch_of(L.wbase, nb, w);
        const int per = L.bh[l].esz / 8, wi = w - L.wbase[l];
        const uint64_t ob = L.bh[l].out ? L.bh[l].out : L.bh[l].elems;
        unsigned long long *d = reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(ob) +
                                                                       (int64_t)L.lo[l] * L.bh[l].esz) + wi;
        __hip_atomic_store(d, (unsigned long long)reinterpret_cast<const uint64_t *>(L.sel)[(L.base[l] + wi / per) * 8 + wi % per],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (pr) p.prof[4] = wall_clock64();
    if (tid == 0) {
        __hip_atomic_store(p.flags + g, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// One launch, its headers in the kernel arguments
__global__ __launch_bounds__(kHpThreads) void k_hpart(HostPartLaunch p)
{
    __shared__ HpLds L;
    const int tid = threadIdx.x, g = blockIdx.x, nb = p.n_batches;
    if (p.c.prof && g == 0 && tid == 0) p.c.prof[0] = wall_clock64();
    if (tid < nb) {
        L.bh[tid] = p.hdr[tid];
        L.prow[0][tid] = p.part[g][tid];
        L.prow[1][tid] = p.part[g + 1][tid];
    }
    __syncthreads();
    hp_scan(L, nb);
    __syncthreads();
    hp_partition(p.c, L, g, nb, p.seq);
}

// The serving kernel: workgroup g takes partition g of every launch published in the pinned ring,
// in order, from p.start[g] on -- no kernel launch per combined batch. Thread 0 polls the next
// slot's seq (uncached, backing off with s_sleep); the workgroup leaves when the host raises *stop,
// after idle_ticks without a launch, or once life_ticks have passed (then between launches), and
// records p.epoch in exited[g] so the host knows to launch a new server for what it publishes next.
__global__ __launch_bounds__(kHpThreads) void k_hserve(HostServeLaunch p)
{
    __shared__ HpLds L;
    const int tid = threadIdx.x, g = blockIdx.x;
    uint32_t next = p.start[g];
    const uint64_t t0 = wall_clock64();
    uint64_t idle_since = t0;
    for (;;) {
        const HostRingSlot *sl = p.ring + (next % (uint32_t)p.ring_n);
        constexpr int HW = (int)(sizeof(HostPartHdr) / 8);
        if (p.spec) {   // thread 0 polls alone; the scan below runs beside the first launch's header loads
            if (tid == 0) {
                int cmd = 0;
                for (;;) {
                    if (ld_sys32(&sl->seq) == next) {
                        cmd = 1;
                        break;
                    }
                    const uint64_t now = wall_clock64();
                    if (ld_sys32(p.stop) || now - idle_since > p.idle_ticks || now - t0 > p.life_ticks) {
                        cmd = 2;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(4);
                }
                L.cmd = cmd;
            }
            __syncthreads();
            if (L.cmd == 2) break;
        }
        if (tid < 64) {
            int cmd = 1;
            if (!p.spec) {
                if (tid == 0) {
                    for (;;) {
                        if (ld_sys32(&sl->seq) == next) {
                            cmd = 1;
                            break;
                        }
                        const uint64_t now = wall_clock64();
                        if (ld_sys32(p.stop) || now - idle_since > p.idle_ticks || now - t0 > p.life_ticks) {
                            cmd = 2;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(4);
                    }
                    L.cmd = cmd;
                }
                cmd = __shfl(cmd, 0);
            }
            if (cmd == 1) {   // this launch and the ones published after it while their batches fit: lane k
                              // reads launch next + k's seq and batch count, all loads in flight together
                const HostRingSlot *sk = p.ring + ((next + (uint32_t)tid) % (uint32_t)p.ring_n);
                const bool in = tid < p.merge;
                const uint32_t sq = in && tid > 0 ? ld_sys32(&sk->seq) : next;
                // the count only once the seq is seen (the host writes a slot's contents before its seq)
                const int nbk = in && sq == next + (uint32_t)tid ? (int)ld_sys32(&sk->n_batches) : 0;
                int incl = nbk;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int v = __shfl_up(incl, d, 64);
                    if (tid >= d) incl += v;
                }
                const bool ok = in && sq == next + (uint32_t)tid && (tid == 0 || incl <= kPartMaxB);
                const uint64_t stop = __ballot(!ok);   // the first launch not taken (lane 0 always is)
                const int nm = stop ? __ffsll((long long)stop) - 1 : 64;
                if (tid < nm) L.sb[tid + 1] = incl;
                if (tid == 0) {
                    L.sb[0] = 0;
                    L.nm = nm;
                }
            }
        } else if (p.spec) {   // launch `next` is published: all kPartMaxB of its headers and rows g, g + 1
            const int u = tid - 64;
            if (u < HW * kPartMaxB) {
                reinterpret_cast<uint64_t *>(L.bh)[u] = ld_sys64(reinterpret_cast<const uint64_t *>(sl->hdr) + u);
            } else if (u < HW * kPartMaxB + 2 * kPartMaxB) {
                const int q = u - HW * kPartMaxB, row = q / kPartMaxB, b = q % kPartMaxB;
                L.prow[row][b] = (uint16_t)ld_sys_u16(&sl->part[g + row][b]);
            }
        }
        __syncthreads();
        if (L.cmd == 2) break;
        const bool pr = p.c.prof && g == 0 && tid == 0;
        const uint64_t t_seen = pr ? wall_clock64() : 0;
        const int nm = L.nm, nbt = L.sb[nm];
        // the headers (8 bytes per thread) and part rows g and g + 1 (2 bytes per thread) of every launch
        // taken, its batches after the previous launch's (p.spec: the first launch's came beside the scan)
        const int bfrom = p.spec ? L.sb[1] : 0;
        if (bfrom < nbt) {
            if (tid >= HW * bfrom && tid < HW * nbt) {
                const int b = tid / HW;
                int k = 0;
                while (L.sb[k + 1] <= b) ++k;
                const HostRingSlot *sk = p.ring + ((next + (uint32_t)k) % (uint32_t)p.ring_n);
                reinterpret_cast<uint64_t *>(L.bh)[tid] =
                    ld_sys64(reinterpret_cast<const uint64_t *>(sk->hdr) + (tid - HW * L.sb[k]));
            } else if (tid >= 128 && tid < 128 + 2 * nbt) {
                const int q = tid - 128, row = q / nbt, b = q % nbt;
                if (b >= bfrom) {
                    int k = 0;
                    while (L.sb[k + 1] <= b) ++k;
                    const HostRingSlot *sk = p.ring + ((next + (uint32_t)k) % (uint32_t)p.ring_n);
                    L.prow[row][b] = (uint16_t)ld_sys_u16(&sk->part[g + row][b - L.sb[k]]);
                }
            }
            __syncthreads();
        }
        if (tid == 0) {   // partition g of the taken launches within kPartCap elements (the first always is)
            int k = 1, tot = 0;
            for (int b = 0; b < L.sb[1]; ++b) tot += L.prow[1][b] - L.prow[0][b];
            for (; k < nm; ++k) {
                int c = 0;
                for (int b = L.sb[k]; b < L.sb[k + 1]; ++b) c += L.prow[1][b] - L.prow[0][b];
                if (tot + c > kPartCap) break;
                tot += c;
            }
            L.nm = k;
        }
        __syncthreads();
        const int taken = L.nm, nb = L.sb[taken];
        hp_scan(L, nb);
        __syncthreads();
        hp_partition(p.c, L, g, nb, next + (uint32_t)taken - 1u);
        if (pr) {   // HKV_PART_PROF: workgroup 0's phase sums over the launches it served (debug)
            unsigned long long *q = p.c.prof;
            q[8] += t_seen - idle_since;
            q[9] += q[1] - t_seen;
            q[10] += q[2] - q[1];
            q[11] += q[3] - q[2];
            q[12] += q[4] - q[3];
            q[13] += 1;
        }
        next += (uint32_t)taken;
        idle_since = wall_clock64();
        __syncthreads();   // LDS reuse by the next launch
    }
    if (tid == 0) __hip_atomic_store(p.exited + g, p.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

static unsigned long long *g_serve_prof = nullptr;
static void serve_prof_print()
{
    const unsigned long long *q = g_serve_prof;
    const double n = q[13] ? (double)q[13] : 1.0;
    fprintf(stderr, "[hkv] k_hserve phases (us, avg of %llu launches, workgroup 0): wait %.2f headers %.2f load+lookup %.2f "
            "rounds %.2f store %.2f\n", q[13], q[8] / n / 100.0, q[9] / n / 100.0, q[10] / n / 100.0, q[11] / n / 100.0,
            q[12] / n / 100.0);
}

int launch_host_serve(const HostServeLaunch &sl0, hipStream_t s)
{
    HostServeLaunch sl = sl0;
    if (getenv("HKV_PART_PROF")) {   // (debug) phase sums, printed at exit
        if (!g_serve_prof) {
            if (hipHostMalloc((void **)&g_serve_prof, 256, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return -3;
            memset(g_serve_prof, 0, 256);
            atexit(serve_prof_print);
        }
        sl.c.prof = g_serve_prof;
    }
    hipLaunchKernelGGL(k_hserve, dim3(kPartG), dim3(kHpThreads), 0, s, sl);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_host_part(const HostPartLaunch &pl, hipStream_t s)
{
    if (pl.n_batches <= 0 || pl.n_batches > kPartMaxB || pl.c.g.entry_size != 64 || pl.c.g.st_value != 31) return -1;
    // HKV_PART_PROF=N: every N-th launch records workgroup 0's phase timestamps and prints the running
    // average (debug; synchronises the stream)
    static const int prof_every = getenv("HKV_PART_PROF") ? atoi(getenv("HKV_PART_PROF")) : 0;
    static unsigned long long *prof = nullptr;
    static long prof_n = 0, k = 0;
    static double sum[4] = {0, 0, 0, 0};
    HostPartLaunch p = pl;
    p.c.prof = nullptr;
    const bool sample = prof_every > 0 && (++prof_n % prof_every) == 0;
    if (sample) {
        if (!prof && hipHostMalloc((void **)&prof, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return -3;
        p.c.prof = prof;
    }
    hipLaunchKernelGGL(k_hpart, dim3(kPartG), dim3(kHpThreads), 0, s, p);
    if (sample) {
        hipStreamSynchronize(s);
        ++k;
        for (int i = 0; i < 4; ++i) sum[i] += (double)(prof[i + 1] - prof[i]) * 10.0 / 1000.0;  // 100 MHz ticks -> us
        fprintf(stderr, "[hkv] k_hpart phases (us, avg of %ld): headers %.2f load+lookup %.2f rounds %.2f store %.2f\n", k,
                sum[0] / k, sum[1] / k, sum[2] / k, sum[3] / k);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

__global__ void k_node_suspected(const uint8_t *elems, const int32_t *ns_idx, int32_t *out, int32_t n_batches,
                                 int32_t stride, int32_t esz, const int32_t *offsets)
{
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_batches) return;
    const int32_t i = ns_idx[b];
    const int64_t base = offsets ? (int64_t)offsets[b] : (int64_t)b * stride;
    if (i >= 0) out[b] = elems[(base + i) * esz + kOpValueOff];
}

// ------------------------------------------------------------------ host side
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The per-launch scratch of cap elements, laid out once: each array 256-byte aligned, in this order from base.
// Returns the bytes taken.
static size_t carve(BatchLaunch &bl, uintptr_t base, int64_t cap, uint32_t entry_size)
{
    uintptr_t p = base;
    auto take = [&](size_t bytes) {
        uint8_t *r = reinterpret_cast<uint8_t *>(p);
        p += align256(bytes);
        return r;
    };
    bl.ent = reinterpret_cast<uint32_t *>(take(4 * (size_t)cap));
    bl.st = take((size_t)cap);
    bl.mem = reinterpret_cast<unsigned long long *>(take(16 * (size_t)cap));
    bl.fbl = reinterpret_cast<uint32_t *>(take(4 * (size_t)cap));
    bl.pf = reinterpret_cast<uint32_t *>(take(4 * (size_t)cap));
    bl.shadow = take((size_t)entry_size * (size_t)cap);
    bl.ctr = reinterpret_cast<uint32_t *>(take(256));
    bl.hx = reinterpret_cast<uint64_t *>(take(16 * (size_t)cap));
    bl.fk = reinterpret_cast<uint16_t *>(take(2 * (size_t)cap));
    bl.cap = (uint32_t)cap;
    return (size_t)(p - base);
}

// the size is the carve from address zero of a launch nobody uses
size_t batch_scratch_bytes(int64_t cap, uint32_t entry_size)
{
    BatchLaunch bl{};
    return carve(bl, 0, cap, entry_size);
}

void batch_carve(BatchLaunch &bl, uint8_t *base, int64_t cap, uint32_t entry_size)
{
    carve(bl, reinterpret_cast<uintptr_t>(base), cap, entry_size);
}

size_t batch_fw_words(uint64_t log_cap) { return (size_t)(log_cap >> 6); }

uint32_t batch_max_epoch() { return (1u << 29) - 1; }

// ---- the plan: which engine runs a launch
// Every predicate on a launch's geometry and flags is written here, once: launch_batch follows the plan, and
// batch_inline_capable tells the runtime which launches have inline instances (the kernels a configs[1] round
// runs). The engines are tested for in the order of Engine's members.
static BatchPlan plan_batch(const BatchLaunch &bl)
{
    BatchPlan p{};
    const int64_t n = bl.n;
    if (n <= 0) return p;   // nothing runs (and nothing has an inline instance)
    const int32_t type = bl.type;
    const uint32_t sv = bl.g.st_value;
    const bool rmw = bl.g.rmw_enabled != 0;
    const bool geo64 = sv == 31 && bl.g.entry_size == 64;   // the default layout: 31-B values in 64-B entries
    const bool local_type = type == kLocal || type == kLocalAfterMemb;
    p.sv = sv == 31 ? 31 : sv == 287 ? 287 : 0;
    p.big = bl.esz > 64;
    p.mixed = bl.hdr != nullptr;
    p.il = bl.line != nullptr;
    p.inv_direct = type == kInvs && !rmw && n < kInvDirectMax;
    p.ack_direct = type == kAcks && !rmw && n < (int64_t)kNone;
    p.ack_out = bl.ack_out && (type == kInvs || (type == kAcks && bl.n_rows > 0));
    p.state_out = local_type;
    p.opc = type == kLocal;
    p.fk = type == kLocal && rmw && p.big;
    p.rw_mirrors = type == kAcks;

    if ((bl.path == kPathSmall || (bl.path == kPathAuto && n <= kSmallMaxElems)) && n <= kSmallMaxElems) {
        p.engine = Engine::kSmall;
    } else if (type == kLocal && !rmw && bl.esz == 56 && geo64 && !bl.offsets) {
        // local batches without RMWs in the default layout
        p.engine = Engine::kLocalDirect;
        p.inline_instance = true;
    } else if (bl.n_rows > 0 && bl.unique) {   // HKV_BATCH_ROWS: one pass over positions of all rows
        p.engine = Engine::kRows;
        p.rmax = bl.n_rows <= 2 ? 2 : 8;
        // elements of 16 B (ACKs without RMWs) keep one chunk each in LDS, others four
        p.ch = type == kInvs ? 4 : bl.esz <= 16 ? 1 : 4;
        // (k_unique_rows: 64-B entries and elements, checked by the runtime)
        p.inline_instance = geo64 && !local_type && bl.n_rows <= 8;
    } else if (bl.unique && (type == kInvs || type == kAcks)) {   // one pass: every key has one element
        if (geo64 && bl.esz <= 64) {
            p.engine = Engine::kUniqueLds64;
            p.inline_instance = true;
        } else if (type == kInvs && sv == 287 && bl.g.entry_size == 320 && bl.esz <= 320) {
            // big-object INVs, whose raises copy 287-B values: staged through LDS (cfg3: 460 -> 326 us per
            // round). ACKs touch the header and the meta only, so they stay in place (LDS-staged: 110 -> 191 us)
            p.engine = Engine::kUniqueLdsBig;
        } else {   // big-entry ACKs, other geometries
            p.engine = Engine::kUniqueInPlace;
            if (p.ack_out) p.refuse = -1;   // only the LDS-staged passes write the ACKs
        }
    } else if (type == kVals) {   // one pass (see k_lookup)
        p.engine = Engine::kValsOnePass;
        p.inline_instance = geo64;
    } else {
        // The head split pays off where one launch piles many candidates onto a few keys: local
        // batches under Zipf. A replica's INVs and ACKs carry at most one write per key and peer per
        // round, so those launches take one pass (their launch-sized head took ~9 us at cfg2).
        p.lookup_head = local_type && n > kLookupHead ? kLookupHead : n;
        p.slab_threads = p.big ? 128 : 256;
        // big ops: local and ACK launches resolve round 0 in place (measured at cfg3: local 1.26 ->
        // 1.05 ms, ACK 0.69 -> 0.55 ms); INV launches keep the LDS slab (0.40 vs 0.52 ms in place)
        p.engine = p.ack_direct ? Engine::kRoundsAckDirect
                   : p.inv_direct ? Engine::kRoundsInvDirect
                   : p.big && type != kInvs ? Engine::kRoundsInPlace
                                            : Engine::kRoundsSlab;
    }
    if (p.il && !p.inline_instance) p.refuse = -1;
    if (bl.region_bytes && p.engine != Engine::kSmall) p.refuse = -1;   // host-staged launches are small ones
    p.node_suspected = p.engine != Engine::kSmall && type == kInvs && bl.ns_idx && bl.node_suspected;

    // big local launches on the rounds engine (configs[2]): k_lookup reads the patches, k_resolve0_direct writes
    // the patched ops (patch_in_resolve, see there): values of at most 320 bytes, the op's pad after its value
    // within its last 8-byte word
    const uint32_t vend = (uint32_t)kOpValueOff + sv;
    if (!bl.patch) p.patches = Patches::kNone;
    else if (p.engine == Engine::kSmall) p.patches = Patches::kApplyFirst;
    else if (p.engine == Engine::kLocalDirect) p.patches = Patches::kByEngine;
    else if (type == kLocal && p.big && !bl.offsets && sv != 31 && sv <= kPirMaxValue && bl.esz % 8 == 0 &&
             (uint32_t)bl.esz >= vend && (uint32_t)bl.esz <= vend + 8)
        p.patches = Patches::kInResolve;
    else p.patches = Patches::kApplyFirst;
    return p;
}

bool batch_inline_capable(const BatchLaunch &bl) { return plan_batch(bl).inline_instance; }

// The kernels' argument block of one launch; a member nobody sets is zero
static BatchArgs make_args(const BatchLaunch &bl, const BatchPlan &p)
{
#ifdef HKV_DEBUG_MODES
    static const int dbg_env = getenv("HKV_DBG") ? atoi(getenv("HKV_DBG")) : 0;
#else
    constexpr int dbg_env = 0;   // the default build cannot skip work (tools/dbg_modes.sh builds its own)
#endif
    static const int check_unique_env = getenv("HKV_CHECK_UNIQUE") ? atoi(getenv("HKV_CHECK_UNIQUE")) : 0;
    BatchArgs a{};
    a.elems = bl.elems;
    a.counts = bl.counts;
    a.offsets = bl.offsets;
    a.index = bl.index;
    a.log = bl.log;
    a.rw = bl.rw;
    a.ns_idx = bl.ns_idx;
    a.fw = bl.fw;
    a.fx = bl.fx;
    a.fy = bl.fy;
    a.ft = bl.ft;
    a.fw_mask = (uint32_t)((bl.g.log_cap >> 6) - 1);
    a.ent = bl.ent;
    a.st = bl.st;
    a.pf = bl.pf;
    a.shadow = bl.shadow;
    a.mem = bl.mem;
    a.fbl = bl.fbl;
    a.ctr = bl.ctr;
    a.error_flags = bl.error_flags;
    a.g = bl.g;
    a.n = bl.n;
    a.rw_stride = bl.rw_stride;
    a.stride = bl.stride;
    a.esz = bl.esz;
    a.type = bl.type;
    a.rtag0 = bl.epoch << 3;
    a.ltag = (uint8_t)(bl.epoch % 255u + 1u);
    a.rounds = rounds_for(bl.type, bl.g.rmw_enabled != 0);
    a.inv_direct = p.inv_direct;
    a.ack_direct = p.ack_direct;
    a.g_membership = bl.g_membership;
    a.w_ack_init = bl.w_ack_init;
    a.node_suspected = bl.node_suspected;
    a.n_batches = bl.n_batches;
    a.host_src = bl.host_src;
    a.host_dst = bl.host_dst;
    a.dev_region = bl.dev_region;
    a.region_bytes = bl.region_bytes;
    a.done_flag = bl.done_flag;
    a.done_value = bl.done_value;
    a.hdr = bl.hdr;
    a.state_out = p.state_out ? bl.state_out : nullptr;
    a.opc = p.opc ? bl.opcode_in : nullptr;
    a.patch = p.patches == Patches::kInResolve || p.patches == Patches::kByEngine ? bl.patch : nullptr;
    a.fk = p.fk ? bl.fk : nullptr;
    a.hx = p.patches == Patches::kInResolve ? bl.hx : nullptr;
    a.rws = p.rw_mirrors ? bl.rw_state : nullptr;
    a.rwo = p.rw_mirrors ? bl.opcode_in : nullptr;
    a.n_rows = bl.n_rows;
    a.skip_row = bl.skip_row;
    a.row_stride = bl.row_stride;
    a.dbg = dbg_env;
    a.check_unique = check_unique_env;
    a.ack_out = p.ack_out ? bl.ack_out : nullptr;
    a.ack_out_size = bl.ack_out_size;
    a.line = bl.line;
    return a;
}

// ---- the engines' launchers; each returns 0 or launch_batch's -3
// k_unique_rows: two positions per lane group, 32 per wave
constexpr int kRowsElems = 16 * kLookupPair;   // positions per k_unique_rows block (its E)
// From kRowsWidePositions on, two-row launches of 16-B ACKs take four positions per lane group, 64 per wave.
// The two-position instance holds 28 blocks on a CU (hipOccupancyMaxActiveBlocksPerMultiprocessor; 7 waves per
// SIMD), 7,168 on the chip's 256 CUs: up to 7,168 * 32 positions every block is resident at once, and smaller
// blocks mean more chains in flight per position. One block more starts only when a first one retires and pays
// the whole dependent chain again on an emptying chip -- a round's ACK launch at configs[1] was 8,390 such
// blocks, 38.4-39.6 us against 34.0 in 4,198 blocks of 64 (5 waves per SIMD, 5,120 resident;
// profiles/ack_rows_kernels.txt, profiles/ack_rows_registers.txt).
constexpr int kRowsWideElems = 16 * 4;
constexpr int64_t kRowsWidePositions = (int64_t)28 * 256 * kRowsElems + 1;
template <int T, int CH>
static void launch_rows(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    const unsigned lgrid = (unsigned)((a.n + kRowsElems - 1) / kRowsElems);
    with_bool(p.il, [&](auto il) {
        constexpr bool IL = decltype(il)::value;
        if constexpr (T == kAcks && CH == 1) {
            if (p.rmax == 2 && a.n >= kRowsWidePositions) {
                const unsigned wgrid = (unsigned)((a.n + kRowsWideElems - 1) / kRowsWideElems);
                hipLaunchKernelGGL((k_unique_rows<T, 2, CH, 4, IL>), dim3(wgrid), dim3(64), 0, s, a);
                return;
            }
        }
        if (p.rmax == 2) {
            hipLaunchKernelGGL((k_unique_rows<T, 2, CH, kLookupPair, IL>), dim3(lgrid), dim3(64), 0, s, a);
        } else {
            hipLaunchKernelGGL((k_unique_rows<T, 8, CH, kLookupPair, IL>), dim3(lgrid), dim3(64), 0, s, a);
        }
    });
}

// the in-place pass and the 64-B LDS-staged one: one element per lane group (16 per wave). Same box, INV phase
// per step (runs r04m, r04t): 72-77 us at 1 element per lane group, 78-80 at 2, 91 at 4
template <int T>
static void launch_unique_t(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    if (p.engine == Engine::kUniqueLds64) {
        const unsigned g1 = (unsigned)((a.n + 15) / 16);
        with_bool(p.il, [&](auto il) {
            hipLaunchKernelGGL((k_unique_lds<T, decltype(il)::value>), dim3(g1), dim3(64), 0, s, a);
        });
    } else {
        const unsigned ugrid1 = (unsigned)((a.n + 63) / 64);
        with_sv(p.sv, [&](auto v) {
            hipLaunchKernelGGL((k_unique<T, decltype(v)::value>), dim3(ugrid1), dim3(256), 0, s, a);
        });
    }
}

static int launch_unique(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    if (p.engine == Engine::kRows) {
        if (a.type == kInvs) launch_rows<kInvs, 4>(a, p, s);
        else if (p.ch == 1) launch_rows<kAcks, 1>(a, p, s);
        else launch_rows<kAcks, 4>(a, p, s);
    } else if (p.engine == Engine::kUniqueLdsBig) {
        hipLaunchKernelGGL(k_unique_big<kInvs>, dim3((unsigned)((a.n + kUbElems - 1) / kUbElems)), dim3(64), 0, s, a);
    } else if (a.type == kInvs) {
        launch_unique_t<kInvs>(a, p, s);
    } else {
        launch_unique_t<kAcks>(a, p, s);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// Round 0's resolve, the rounds, the commit and the fallback of one (batch type, value class)
template <int T, int V>
static int launch_rounds_tv(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    const unsigned grid = (unsigned)((a.n + 255) / 256);
    const unsigned cgrid = (unsigned)((a.n + 256 * kCandPer - 1) / (256 * kCandPer));
    const unsigned rgrid = (unsigned)((a.n + p.slab_threads - 1) / p.slab_threads);
    const size_t rlds = (size_t)p.slab_threads * (size_t)a.esz;
    if (p.big && rlds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)k_resolve0<T, V, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds) !=
            hipSuccess)
        return -3;
    if (p.engine == Engine::kRoundsInPlace) hipLaunchKernelGGL((k_resolve0_direct<T, V>), dim3(grid), dim3(256), 0, s, a);
    else if (p.big) hipLaunchKernelGGL((k_resolve0<T, V, 128>), dim3(rgrid), dim3(128), rlds, s, a);
    else hipLaunchKernelGGL((k_resolve0<T, V, 256>), dim3(rgrid), dim3(256), rlds, s, a);
    for (int r = 1; r <= a.rounds; ++r) {
        hipLaunchKernelGGL((k_cand<T>), dim3(cgrid), dim3(256), 0, s, a, r);
        hipLaunchKernelGGL((k_resolve<T, V>), dim3(grid), dim3(256), V == 31 ? 256 * a.esz : 0, s, a, r);
    }
    hipLaunchKernelGGL((k_commit<V>), dim3(grid), dim3(256), 0, s, a);
    if (a.rounds > 0) hipLaunchKernelGGL((k_fb_exec<T, V>), dim3(256), dim3(kFbThreads), 0, s, a);
    return 0;
}

template <int T>
static int launch_rounds_t(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    int rc = 0;
    with_sv(p.sv, [&](auto v) { rc = launch_rounds_tv<T, decltype(v)::value>(a, p, s); });
    return rc;
}

// kValsOnePass and the four rounds engines: all begin with k_lookup, one element per lane group. Same box, VAL
// batch per step (runs r04m, r04u): 49.6-50.2 us at 1, 52.3-53.9 at 2, 57 at 4; configs[2] 0.627-0.635 against
// 0.620-0.622 G ops/s at two (run r04v)
static int launch_rounds(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    const int64_t n = a.n;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (p.engine == Engine::kValsOnePass) {
        with_bool(p.il, [&](auto il) {
            hipLaunchKernelGGL(k_lookup<decltype(il)::value>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, a,
                               (int64_t)0, n);
        });
        return hipGetLastError() == hipSuccess ? 0 : -3;
    }
    const int64_t head = p.lookup_head;
    hipLaunchKernelGGL(k_lookup<>, dim3((unsigned)((head + 63) / 64)), dim3(256), 0, s, a, (int64_t)0, head);
    if (n > head) hipLaunchKernelGGL(k_lookup<>, dim3((unsigned)((n - head + 63) / 64)), dim3(256), 0, s, a, head, n);
    int rc = 0;
    if (p.engine == Engine::kRoundsAckDirect) {
        hipLaunchKernelGGL(k_ack_resolve, dim3(grid), dim3(256), 0, s, a);
    } else if (p.engine == Engine::kRoundsInvDirect) {
        hipLaunchKernelGGL(k_inv_resolve, dim3(grid), dim3(256), 0, s, a, (int64_t)0, n);
        with_sv(p.sv, [&](auto v) { hipLaunchKernelGGL((k_inv_commit<decltype(v)::value>), dim3(grid), dim3(256), 0, s, a); });
    } else {
        switch (a.type) {
        case kLocal: rc = launch_rounds_t<kLocal>(a, p, s); break;
        case kLocalAfterMemb: rc = launch_rounds_t<kLocalAfterMemb>(a, p, s); break;
        case kInvs: rc = launch_rounds_t<kInvs>(a, p, s); break;
        case kAcks: rc = launch_rounds_t<kAcks>(a, p, s); break;
        default: rc = launch_rounds_t<kVals>(a, p, s); break;
        }
    }
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_batch(BatchLaunch &bl, hipStream_t s)
{
    if (bl.n <= 0) return 0;
    const BatchPlan p = plan_batch(bl);
    if (p.refuse) return p.refuse;
    const BatchArgs a = make_args(bl, p);
    if (p.patches == Patches::kApplyFirst)   // the patches as op writes first, then the launch as usual
        hipLaunchKernelGGL(k_apply_patch, dim3((unsigned)((bl.n + 255) / 256)), dim3(256), 0, s, bl.elems, bl.patch, bl.n,
                           bl.esz, bl.g.st_value);
    int rc;
    switch (p.engine) {
    case Engine::kSmall: rc = launch_small(a, p, s); break;
    case Engine::kLocalDirect: rc = launch_local(a, p, s); break;
    case Engine::kRows:
    case Engine::kUniqueLds64:
    case Engine::kUniqueLdsBig:
    case Engine::kUniqueInPlace: rc = launch_unique(a, p, s); break;
    default: rc = launch_rounds(a, p, s); break;   // kValsOnePass and the rounds
    }
    if (rc) return rc;
    if (p.node_suspected) {
        hipLaunchKernelGGL(k_node_suspected, dim3((bl.n_batches + 255) / 256), dim3(256), 0, s, bl.elems, bl.ns_idx,
                           bl.node_suspected, bl.n_batches, bl.stride, bl.esz, bl.offsets);
        if (hipGetLastError() != hipSuccess) return -4;
    }
    return 0;
}

}  // namespace hkv
