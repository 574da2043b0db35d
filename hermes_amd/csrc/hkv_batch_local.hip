// hkv_batch_local.hip -- the batch path's direct local engine (Engine::kLocalDirect) and its launcher.
//
// Local batches without RMWs, 56-B ops and 64-B entries (configs[1]). Under these, an element's
// key can only be mutated by a PUT (hermes_exec_write) from VALID/INVALID, or by a GET replay
// from INVALID (hermes_exec_read -> write replay), and its first mutation leaves the key in an
// absorbing state (WRITE/REPLAY, see absorbing_state). So every element's result is fixed by S_0
// and by F, its key's first mutating element:
//   i < F (or no F): the exec function against S_0;  i = F: S_0 -> its shadow;  i > F: against WRITE.
// Three passes instead of lookup + re-reading every op and entry line:
//   k_local_pre    the PUTs only (one op header per element, then bucket + log line per PUT):
//                  every PUT that mutates S_0 offers F and tags its entry's seqlock byte;
//   k_local_fused  every element: op slab through LDS, bucket, log line (the whole 64-B entry, four
//                  lanes) -- F is final for every key not INVALID at S_0, so each element resolves
//                  right there, F applies itself to its shadow, and the slab is written back once;
//                  elements of INVALID keys (where GET replays may mutate: they offer F here) wait;
//   k_local_deferred  those waiting elements, against the final F.
// k_commit_w then installs the shadows. Measured against k_lookup + k_resolve0: the entry line and
// the op slab are read once instead of twice.
#include <hip/hip_runtime.h>

#include "hkv_batch_dev.h"

namespace hkv {

// work-skipping timing modes of k_local_pre and k_local_fused (tools/dbg_modes.sh): compiled in only with
// -DHKV_DEBUG_MODES; the default build folds every test to false
#ifdef HKV_DEBUG_MODES
#define HKV_DBG_ON(a, bit) (((a).dbg & (bit)) != 0)
#else
#define HKV_DBG_ON(a, bit) false
#endif

// Round 5: 2048 elements per block (512 threads), a 2048-slot table: each block looks up and offers
// each of its PUT keys once, so doubling the block removes the second lookup of the keys two 1024-element
// halves shared, and the two head elements per thread instead of four cut registers. Same box, 3 x 20
// steps (run r05v): prepass 76.1 -> 64.2 us, 4.25-4.29 -> 4.27-4.36 G ops/s; 1536 (86 us), 4096 (78 us),
// a 2048-element head (79 us) and a 4096-slot table (111 us) were slower
constexpr int kPreElems = 2048;            // elements per k_local_pre block
constexpr int kPreThreads = kPreElems / 4; // four of its own elements per thread
constexpr int kPreHead = 1024;             // launch head whose PUT keys every block knows
constexpr int kPreHash = 2048;             // LDS slots of a (key -> first PUT) table (a power of two)

// Inline instances (IL): an entry id of the local launch's scratch carries "this key's entry lives in its
// bucket's line" in bit 31 (ids stay below it while log_cap <= kInlineMaxLog). A key's identity -- F/X/Y/T
// words, phys_of, fw_index -- stays its log offset; only the bytes' home differs, and that is a function of the
// bucket, so of the key, which every element, entry image and shadow holds.
constexpr uint32_t kEntInline = 0x80000000u;
template <bool IL>
__device__ __forceinline__ uint32_t ent_id(uint32_t e) { return IL ? e & ~kEntInline : e; }
template <bool IL>
__device__ __forceinline__ uint8_t *entry_home(const BatchArgs &a, uint32_t e, uint64_t key)
{
    if (IL && (e & kEntInline)) return line_entry(a.line, a.g, key);
    return entry_of(a, ent_id<IL>(e));
}

// the key of element i as the launch sees it (patched or not)
__device__ __forceinline__ uint64_t elem_key(const BatchArgs &a, int64_t i)
{
    if (a.patch && a.patch[i * 16 + 14]) return *reinterpret_cast<const uint64_t *>(a.patch + i * 16);
    return *reinterpret_cast<const uint64_t *>(a.elems + i * a.esz);
}

// a patch applied to the 16-B chunk q (bytes 16q..16q+15) of a 56-B op with a 31-B value
__device__ __forceinline__ uint4 patch_chunk(uint4 w, int q, uint64_t pa, uint64_t pb)
{
    const uint32_t fill = (uint32_t)((pb >> 32) & 0xFFu) * 0x01010101u;
    const bool vfill = fill != 0, reset = ((pb >> 40) & 0xFFu) != 0;
    if (q == 0) {
        w.x = (uint32_t)pa;
        w.y = (uint32_t)(pa >> 32);
        // opcode, ST_NEW, val_len; ts.cid (byte 11) and ts.version (12..15) kept unless reset
        w.z = (uint32_t)(pb & 0xFFu) | ((uint32_t)kNew << 8) | ((uint32_t)((pb >> 8) & 0xFFu) << 16) |
              (reset ? 0u : (w.z & 0xFF000000u));
        if (reset) w.w = 0;
    } else if (q == 1) {
        const uint32_t flags = (uint32_t)((pb >> 16) & 0xFFFFu);
        w.x = flags | (vfill ? (fill & 0xFFFF0000u) : (w.x & 0xFFFF0000u));
        if (vfill) w.y = w.z = w.w = fill;
    } else if (q == 2) {
        if (vfill) w.x = w.y = w.z = w.w = fill;
    } else if (vfill) {  // bytes 48..55: byte 48 is the value's last
        w.x = (w.x & 0xFFFFFF00u) | (fill & 0xFFu);
    }
    return w;
}

__device__ __forceinline__ uint32_t pre_slot(uint64_t key)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - __builtin_ctz(kPreHash))) & (kPreHash - 1);
}

// (key -> smallest element) in an LDS table of kPreHash slots, key ~0 the empty mark; false when the
// key cannot go in (key ~0 itself, or a full table)
__device__ __forceinline__ bool pre_insert(uint64_t *hk, uint32_t *hv, uint64_t key, uint32_t i, bool &created,
                                           uint32_t &slot)
{
    created = false;
    if (key == ~0ull) return false;
    uint32_t sl = pre_slot(key);
    for (int n = 0; n < kPreHash; ++n) {
        const unsigned long long old = atomicCAS((unsigned long long *)&hk[sl], ~0ull, key);
        if (old == ~0ull || old == key) {
            created = old == ~0ull;
            atomicMin(&hv[sl], i);
            slot = sl;
            return true;
        }
        sl = (sl + 1) & (kPreHash - 1);
    }
    return false;
}

// a key into an LDS set of kPreHash slots (the head's PUT keys: only membership is asked)
__device__ __forceinline__ void pre_insert_key(uint64_t *hk, uint64_t key)
{
    if (key == ~0ull) return;
    uint32_t sl = pre_slot(key);
    for (int n = 0; n < kPreHash; ++n) {
        const unsigned long long old = atomicCAS((unsigned long long *)&hk[sl], ~0ull, key);
        if (old == ~0ull || old == key) return;
        sl = (sl + 1) & (kPreHash - 1);
    }
}

// The PUTs of kPreElems elements offer F. Whether a PUT mutates S_0 depends on S_0 alone
// (hermes_exec_write: VALID or INVALID and no op buffer index), so either every PUT of a key is a
// candidate or none is, and F is the key's first PUT or nothing. So each block looks up each key
// once, for its first PUT (an LDS table of the block's PUT keys). A Zipf-hot key's PUTs are spread
// over every block, and all blocks of the launch are in flight together: every block also reads the
// keys of the PUTs among the launch's first kPreHead elements (before its own; headers only,
// L2-resident after the first block) and drops its keys that have a PUT there -- an earlier block
// offers that one. Four keys per lane group are in flight; the offer is a plain atomicMin.
constexpr int kPrePair = 4;   // keys per lane group in flight in the prepass's lookups (2 or 8 were slower: DESIGN 6,
                              // round 5). No occupancy or SGPR attribute: neither moved the prepass
// No seqlock-byte tags (round 5): k_local_fused loads every hit's F word beside its log line and needs
// no mark of the keys that have one
template <bool IL = false>
__global__ __launch_bounds__(kPreThreads) void k_local_pre(BatchArgs a)
{
    constexpr int HEAD = kPreHead;
    __shared__ uint64_t hk[kPreHash], gk[kPreHash];  // the block's PUT keys, the head's
    __shared__ uint32_t hv[kPreHash];
    __shared__ uint32_t dl[kPreElems];               // distinct keys: slots of hk, or ~index (no slot)
    __shared__ uint32_t nd;
    const int tid = threadIdx.x, q = tid & 3, gbase = (tid & 63) & ~3;
    if (tid == 0) {
        nd = 0;
        if (blockIdx.x == 0) a.ctr[kCtrDefer] = 0;
    }
    for (int j = tid; j < kPreHash; j += kPreThreads) {
        hk[j] = ~0ull;
        gk[j] = ~0ull;
        hv[j] = kNone;
    }
    if (HKV_DBG_ON(a, 8)) return;
    const int64_t i0 = (int64_t)blockIdx.x * kPreElems;
    const int64_t head_end = HKV_DBG_ON(a, 4) ? 0 : i0 < HEAD ? i0 : HEAD;  // the head: elements before the block's own
    // PUTs that are not skipped (hermes_skip_op, hermesKV.c:709-769). Reading every op header is a
    // pass over the whole op slab; with the caller's opcode mirror only the PUTs' headers are read
    // (the others read element 0's, one cached line; k_local_fused checks the mirror against every
    // element's opcode). Loads are unconditional and all issued before the first is used.
    constexpr int kOwnK = kPreElems / kPreThreads, kAllK = kOwnK + (HEAD + kPreThreads - 1) / kPreThreads;
    U64x2 h[kAllK];
    bool in[kAllK];
    uint8_t opm[kAllK];
    U64x2 pt[kAllK];
#pragma unroll
    for (int k = 0; k < kAllK; ++k) {
        const bool own = k < kOwnK;
        const int64_t i = own ? i0 + k * kPreThreads + tid : (int64_t)(k - kOwnK) * kPreThreads + tid;
        in[k] = i < a.n && (own || i < head_end);
        opm[k] = a.opc ? a.opc[in[k] ? i : 0] : (uint8_t)kOpPut;
    }
    if (a.patch) {
        // the patches first: a refilled PUT's patch holds all the prepass needs (key, opcode, ST_NEW),
        // so only the PUTs kept from the last round read their op header (a second dependent load
        // for them, against a third of the op slab's lines fetched for nothing)
#pragma unroll
        for (int k = 0; k < kAllK; ++k) {
            const bool own = k < kOwnK;
            const int64_t i = own ? i0 + k * kPreThreads + tid : (int64_t)(k - kOwnK) * kPreThreads + tid;
            pt[k] = in[k] && opm[k] == kOpPut ? *reinterpret_cast<const U64x2 *>(a.patch + i * 16) : U64x2{0, 0};
        }
#pragma unroll
        for (int k = 0; k < kAllK; ++k) {
            const bool own = k < kOwnK;
            const int64_t i = own ? i0 + k * kPreThreads + tid : (int64_t)(k - kOwnK) * kPreThreads + tid;
            h[k] = *reinterpret_cast<const U64x2 *>(a.elems + (in[k] && opm[k] == kOpPut && !patch_valid(pt[k].b) ? i : 0) * 56);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kAllK; ++k) {
            const bool own = k < kOwnK;
            const int64_t i = own ? i0 + k * kPreThreads + tid : (int64_t)(k - kOwnK) * kPreThreads + tid;
            h[k] = *reinterpret_cast<const U64x2 *>(a.elems + (in[k] && opm[k] == kOpPut ? i : 0) * 56);
            pt[k] = U64x2{0, 0};
        }
    }
#pragma unroll
    for (int k = 0; k < kAllK; ++k)
        if (patch_valid(pt[k].b)) {   // a patched element: its key and opcode, state ST_NEW
            h[k].a = pt[k].a;
            h[k].b = (h[k].b & ~0xFFFFull) | (pt[k].b & 0xFFu) | ((uint64_t)kNew << 8);
        }
#pragma unroll
    for (int k = 0; k < kAllK; ++k) {
        const bool own = k < kOwnK;
        const int64_t i = own ? i0 + k * kPreThreads + tid : (int64_t)(k - kOwnK) * kPreThreads + tid;
        // a non-PUT read element 0's raw header, which a patch may have made stale: only the
        // mirror's PUTs take part
        in[k] = in[k] && opm[k] == kOpPut && in_count(a, (uint32_t)i);
    }
    if (HKV_DBG_ON(a, 16)) {
        uint64_t acc = 0;
#pragma unroll
        for (int k = 0; k < kAllK; ++k) acc += h[k].a ^ h[k].b;
        if (acc == 0x1234567ull) a.ctr[7] = 1;
        return;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kAllK; ++k) {
        const bool own = k < kOwnK;
        const uint32_t i = (uint32_t)(own ? i0 + k * kPreThreads + tid : (int64_t)(k - kOwnK) * kPreThreads + tid);
        const uint64_t key = h[k].a;
        if (!(in[k] && (uint8_t)h[k].b == kOpPut && !skip_elem_os(kLocal, kOpPut, (uint8_t)(h[k].b >> 8)))) continue;
        bool created;
        uint32_t sl;
        if (own) {
            const bool in_table = pre_insert(hk, hv, key, i, created, sl);
            if (!in_table || created) {  // a key's first arrival lists it (no slot: it offers for itself)
                dl[atomicAdd(&nd, 1u)] = in_table ? sl : ~i;
            }
        } else {
            pre_insert_key(gk, key);
        }
    }
    __syncthreads();
    const Ctx c = make_ctx(a);
    const uint64_t hput[2] = {0, (uint64_t)kOpPut};
    const uint32_t cnt = HKV_DBG_ON(a, 2) ? 0 : nd;
    for (uint32_t base = 0; base < cnt; base += (kPreThreads / 4) * kPrePair) {
        uint64_t key[kPrePair];
        bool probe[kPrePair], ok[kPrePair];
        uint32_t idx[kPrePair];
        uint64_t phys[kPrePair];
        uint4 ln[kPrePair];
#pragma unroll
        for (int k = 0; k < kPrePair; ++k) {
            const uint32_t j = base + k * (kPreThreads / 4) + (tid >> 2);
            probe[k] = j < cnt;
            const uint32_t d = probe[k] ? dl[j] : 0u;
            idx[k] = !probe[k] ? kNone : d < (uint32_t)kPreHash ? hv[d] : ~d;
            key[k] = !probe[k] ? 0 : d < (uint32_t)kPreHash ? hk[d] : elem_key(a, (int64_t)idx[k]);
            if (probe[k] && head_end > 0 && key[k] != ~0ull) {  // a head PUT of the key comes first
                uint32_t sl = pre_slot(key[k]);
                for (int n = 0; n < kPreHash; ++n) {
                    const uint64_t g = gk[sl];
                    if (g == ~0ull) break;
                    if (g == key[k]) {
                        probe[k] = false;
                        break;
                    }
                    sl = (sl + 1) & (kPreHash - 1);
                }
            }
        }
        lookup_pair<kPrePair, IL>(a, key, probe, q, gbase, ok, phys, ln);
#pragma unroll
        for (int k = 0; k < kPrePair; ++k) {
            Meta m0;
            const uint64_t ek = line_key_meta(ln[k], m0);
            if (q != 0 || !ok[k] || ek != key[k]) continue;
            if (!would_mutate(kLocal, reinterpret_cast<const uint8_t *>(hput), m0, c) || HKV_DBG_ON(a, 1)) continue;
            atomicMin(a.fw + fw_index(a, phys[k]), ((unsigned long long)(~a.rtag0) << 32) | idx[k]);
        }
    }
}

// exec_read / exec_write (hermesKV.c:251-356, with the skew optimisations of :196-238) for a local op
// of the direct path (RMWs off) that leaves its key's meta m as it is: the caller has excluded the
// branches that change it (update_actions, write replays) -- the element is not its key's first
// mutating element, so would_mutate is false against S_0, or m is the key's meta after that first write
// -- and only the element's own bytes move, without the generic dispatch's meta updates. An element
// that would mutate after all raises error flag bit 0, as the generic path's meta check does.
__device__ __forceinline__ void local_resolve_nm(const BatchArgs &a, uint8_t *x, const uint8_t *ent, const Meta &m)
{
    const uint8_t oc = x[8], st = m_state(m);
    const bool obi_empty = m_obi(m) == kObiEmpty;
    bool mut = false;
    if (oc == kOpGet) {
        if (st == kValid) {
            copy_value<31>(x + kOpValueOff, ent + kEntryValueOff, 31);
            x[9] = kGetComplete;
            x[10] = (uint8_t)((m_val_len(m) >> a.g.shift) - kOpMetaSize);
        } else if (st == kInvalidWrite || st == kWrite || st == kReplay) {
            x[9] = kGetStall;
        } else {
            x[9] = kEmpty;
            if (st == kInvalid) {   // hermes_check_membership_n_write_replay_actions, hermesKV.c:179-194
                const uint8_t lw = m_lwid(m);
                if (lw < 8 && ((a.g_membership >> lw) & 1u)) x[9] = kGetStall;
                else mut = obi_empty;
            }
        }
        if (a.g.skew & kSkewReadComplete) hot_read_complete(x, m.ver, m_cid(m));
    } else if (oc == kOpPut) {
        mut = (st == kValid || st == kInvalid) && obi_empty;
        x[9] = kPutStall;
        if (a.g.skew & kSkewWriteCoalesce) {   // as exec_write (hkv_exec.h)
            const uint32_t cv = m.ver & 0xFFFFu;
            uint32_t over = ld32(x + 12);
            if (st != kReplay && over == 0) {
                st32(x + 12, cv);
                over = cv;
            }
            if (over > 0 && over + 1u < cv) x[9] = kPutComplete;
        }
    }
    if (mut && a.error_flags) atomicOr(a.error_flags, 1u);
}

// F of the direct path: S_0 -> S_1 by the exec function on the element's own LDS copies of op (x) and entry
// (ent, meta m) -- each element has a private copy of its entry, so the image nobody else reads becomes the
// shadow's bytes, which the caller stores to shadow_of(a, i) whole (apply_to_shadow's result without its
// byte accesses to global memory)
__device__ __forceinline__ void local_first_lds(const BatchArgs &a, uint8_t *x, uint32_t i, uint8_t *ent, Meta m)
{
    Ctx c = make_ctx(a);
    // the element's index in its batch (elem_at's, under 2^31 elements: 32-bit division)
    const uint8_t idx = (uint8_t)(i - i / (uint32_t)a.stride * (uint32_t)a.stride);
    if (x[8] == kOpGet) exec_read<31>(x, ent, idx, m, c);
    else if (x[8] == kOpPut) exec_write<31>(x, ent, idx, m, c);
    meta_store(ent, m);
}

// Every element, F final (except on INVALID keys): see the section comment. The lookup runs four
// lanes per element (each lane holds 16 B of the op and of the log line); the LDS copies of op and
// entry are then resolved one element per lane (see NW below); the ops go back whole.
// Every hit's F word is loaded beside its log line; the word alone says whether this launch's prepass
// offered a first candidate for the key (first_cand)
// SGPR budget of k_local_fused, 80 (round 6: local launch 353-355 -> 341-351 us, 7 -> 8 waves per SIMD): waves are admitted
// per SIMD by ~800 SGPRs / (ceil(sgpr/16) * 16 + 16) (MI355X_MICROARCH.md, "Residency"), so 92 SGPRs allow
// 7 waves and 80 allow 8
// NW waves per block (round 6): each wave loads, looks up and stages its own 32 elements, and after the block's
// barrier the stage bytes and the state mirror of all NW * 32 elements go out as whole 64-byte blocks (a
// wave's 32 bytes alone are half a block, which HBM writes with a read-modify-write: tools/calib_bench.hip,
// 16-B random writes 2.4x the time of 64-B ones).
// The resolve runs on full waves: between the barriers wave 0 resolves all 64 elements of the block, one per
// lane, so the divergent exec code is issued once per 64 elements and not once per 32 on half-empty waves. A
// key's first writer runs its exec function on its LDS copy of the entry (local_first_lds) and the wave then
// stores the finished images to their shadows, 16 B per lane ("The fused pass's instructions").
constexpr int kLfWaves = 2;   // waves per k_local_fused block
template <bool IL = false>
__global__ __launch_bounds__(64 * kLfWaves) __attribute__((amdgpu_num_sgpr(80))) void k_local_fused(BatchArgs a)
{
    constexpr int P = 2, NW = kLfWaves;   // elements per lane group, waves per block
    constexpr int E = 16 * P;   // elements per wave: P per lane group
    constexpr int EB = E * NW;  // elements per block
    static_assert(EB == 64, "one wave resolves the block, one element per lane");
    // per block element, each wave staging its own E
    __shared__ uint4 sops_b[EB * 4];      // 64 B per op (56 used)
    __shared__ uint4 sln_b[EB * 4];
    __shared__ unsigned long long sfw_b[EB];
    __shared__ uint32_t sent_b[EB];       // entry id of a hit, kNone otherwise
    __shared__ uint8_t sprb_b[EB];        // probed (not skipped)
    __shared__ uint8_t sfl[EB];           // the block's first writers (F), whose images go to their shadows
    __shared__ uint32_t sst[EB / 4], sstate[EB / 4];   // the block's stage bytes and state mirror
    __shared__ uint32_t sdef[EB];
    __shared__ uint32_t ndef;
    const int w = threadIdx.x >> 6, tid = threadIdx.x & 63, q = tid & 3, gbase = tid & ~3;
    uint4 *sops = sops_b + w * E * 4, *sln = sln_b + w * E * 4;
    unsigned long long *sfw = sfw_b + w * E;
    uint32_t *sent = sent_b + w * E;
    uint8_t *sprb = sprb_b + w * E;
    const int64_t ib = (int64_t)blockIdx.x * EB, i0 = ib + (int64_t)w * E;
    if (threadIdx.x == 0) ndef = 0;
    uint64_t key[P];
    bool probe[P], ok[P], live[P];
    uint64_t phys[P];
    uint4 ln[P], op[P];
    int te[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        te[k] = k * 16 + (tid >> 2);
        const int64_t i = i0 + te[k];
        live[k] = i < a.n;
        op[k] = make_uint4(0u, 0u, 0u, 0u);
        if (live[k]) {
            const uint8_t *xg = a.elems + i * 56 + 16 * q;
            U64x2 p{0, 0};
            if (a.patch) p = *reinterpret_cast<const U64x2 *>(a.patch + i * 16);
            if (q < 3) {
                op[k] = *reinterpret_cast<const uint4 *>(xg);
            } else {
                const uint64_t t = *reinterpret_cast<const uint64_t *>(xg);
                op[k].x = (uint32_t)t;
                op[k].y = (uint32_t)(t >> 32);
            }
            if (patch_valid(p.b)) op[k] = patch_chunk(op[k], q, p.a, p.b);
        }
        sops[te[k] * 4 + q] = op[k];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        // lane 0 of the group holds op bytes 0..15: the key and the header
        key[k] = (uint64_t)(uint32_t)__shfl((int)op[k].x, 0, 4) | ((uint64_t)(uint32_t)__shfl((int)op[k].y, 0, 4) << 32);
        const uint32_t h0 = (uint32_t)__shfl((int)op[k].z, 0, 4);
        probe[k] = false;
        if (live[k] && !HKV_DBG_ON(a, 128))
            probe[k] = in_count(a, (uint32_t)(i0 + te[k])) && !skip_elem_os(kLocal, (uint8_t)h0, (uint8_t)(h0 >> 8));
    }
    unsigned long long fwv[P];   // a hit's F word, loaded beside its log line
    bool inl[P];                 // (IL) the hit is its bucket's inline key
    if (HKV_DBG_ON(a, 512)) {   // (timing modes) no F loads
        lookup_pair<P, IL>(a, key, probe, q, gbase, ok, phys, ln, nullptr, inl);
#pragma unroll
        for (int k = 0; k < P; ++k) fwv[k] = ~0ull;
    } else {
        lookup_pair_f<P, IL>(a, key, probe, q, gbase, ok, phys, ln, fwv, nullptr, inl);
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        Meta m;
        const uint64_t ek = line_key_meta(ln[k], m);
        const bool hit = ok[k] && ek == key[k];
        // keys INVALID at S_0 take their F after this pass (k_local_deferred)
        const unsigned long long f = hit && m_state(m) != kInvalid && q == 0 ? fwv[k] : ~0ull;
        if (hit) sln[te[k] * 4 + q] = ln[k];
        if (q == 0) {
            sfw[te[k]] = f;
            sent[te[k]] = hit ? (uint32_t)(phys[k] / a.g.entry_unit) | (IL && inl[k] ? kEntInline : 0u) : kNone;
            sprb[te[k]] = probe[k];
        }
    }
    __syncthreads();
    // wave 0 resolves the block's EB elements, one per lane, on both waves' LDS copies: the exec code's
    // branches are issued once per 64 elements; wave 1 waits at the barrier
    if (__builtin_amdgcn_readfirstlane(w) == 0 && !HKV_DBG_ON(a, 64)) {
        const int64_t i = ib + tid;
        uint8_t st = kStDone;
        if (i < a.n) {
            uint8_t *x = reinterpret_cast<uint8_t *>(&sops_b[tid * 4]);
            uint8_t *ent = reinterpret_cast<uint8_t *>(&sln_b[tid * 4]);
            const uint32_t e = sent_b[tid];
            const bool prb = sprb_b[tid] != 0;
            if (e != kNone) {
                Meta m;
                meta_load(ent, m);
                Ctx c = make_ctx(a);
                const bool wm = would_mutate(kLocal, x, m, c);
                if (m_state(m) == kInvalid) {
                    // GET replays may mutate: they offer F now, and the key's elements resolve later
                    if (wm) {
                        const uint64_t ph = phys_of(a, ent_id<IL>(e));
                        offer(a.fw + fw_index(a, ph), a.rtag0, (uint32_t)i);
                        if ((uint8_t)(m.w5 >> 16) != a.ltag)
                            entry_home<IL>(a, e, *reinterpret_cast<const uint64_t *>(x))[kEntryMetaOff + 4] = a.ltag;
                    }
                    st = kStDefer;
                    sdef[atomicAdd(&ndef, 1u)] = (uint32_t)i;
                } else {
                    const uint32_t f = first_cand(sfw_b[tid], a.rtag0);
                    // a mutating element must have offered itself in k_local_pre
                    if (wm && (f == kNone || f > (uint32_t)i) && a.error_flags) atomicOr(a.error_flags, 4u);
                    if ((uint32_t)i == f) {
                        local_first_lds(a, x, (uint32_t)i, ent, m);
                        st = kStCommit;
                    } else {
                        // F of a key that is not INVALID is its first PUT (k_local_pre)
                        local_resolve_nm(a, x, ent, f != kNone && (uint32_t)i > f ? after_first<kLocal>(a, m, f, 1) : m);
                    }
                }
            } else if (prb) {
                x[9] = kMiss;
            }
            // k_local_pre read only the PUTs the caller's opcode mirror names
            if (a.opc && prb && x[8] == kOpPut && a.opc[i] != kOpPut && a.error_flags) atomicOr(a.error_flags, 8u);
            if (!HKV_DBG_ON(a, 1024)) a.ent[i] = e;
            // a deferred element's state byte is written again by k_local_deferred, after this pass
            reinterpret_cast<uint8_t *>(sst)[tid] = st;
            reinterpret_cast<uint8_t *>(sstate)[tid] = x[9];
        }
        // the first writers' entry images, finished in LDS, go to their shadows: four lanes per image, 16 B
        // each, 16 images per step
        const unsigned long long fm = __ballot(st == kStCommit);
        if (fm && !HKV_DBG_ON(a, 1024)) {
            if (st == kStCommit) sfl[__popcll(fm & ((1ull << tid) - 1ull))] = (uint8_t)tid;
            __threadfence_block();   // the images and the list, written by this wave's other lanes
            const int nf = __popcll(fm);
            for (int j = tid >> 2; j < nf; j += 16) {
                const int t = sfl[j];
                reinterpret_cast<uint4 *>(shadow_of(a, (uint32_t)(ib + t)))[q] = sln_b[t * 4 + q];
            }
        }
    }
    __syncthreads();
    // the block's stage bytes and state mirror as whole blocks (a partial last block byte by byte)
    if (!HKV_DBG_ON(a, 1024) && !HKV_DBG_ON(a, 64)) {
        if (ib + EB <= a.n && ((uintptr_t)a.state_out & 3) == 0) {   // (st is 256-byte aligned)
            if ((int)threadIdx.x < EB / 4) {
                reinterpret_cast<uint32_t *>(a.st + ib)[threadIdx.x] = sst[threadIdx.x];
                if (a.state_out) reinterpret_cast<uint32_t *>(a.state_out + ib)[threadIdx.x] = sstate[threadIdx.x];
            }
        } else if ((int)threadIdx.x < EB && ib + threadIdx.x < a.n) {
            a.st[ib + threadIdx.x] = reinterpret_cast<const uint8_t *>(sst)[threadIdx.x];
            if (a.state_out) a.state_out[ib + threadIdx.x] = reinterpret_cast<const uint8_t *>(sstate)[threadIdx.x];
        }
    }
    // the waiting elements (keys INVALID at S_0: rare), appended once per block
    if (ndef && threadIdx.x == 0) {
        const uint32_t base = atomicAdd(&a.ctr[kCtrDefer], ndef);
        for (uint32_t j = 0; j < ndef; ++j) a.fbl[base + j] = sdef[j];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (!live[k] || HKV_DBG_ON(a, 256)) continue;
        uint8_t *xg = a.elems + (i0 + te[k]) * 56 + 16 * q;
        const uint4 v = sops[te[k] * 4 + q];
        if (q < 3) *reinterpret_cast<uint4 *>(xg) = v;
        else *reinterpret_cast<uint64_t *>(xg) = (uint64_t)v.x | ((uint64_t)v.y << 32);
    }
}

// Elements of keys that were INVALID at S_0, against their key's final F (k_resolve0_direct's rules)
template <bool IL = false>
__global__ __launch_bounds__(256) void k_local_deferred(BatchArgs a)
{
    const uint32_t nd = a.ctr[kCtrDefer];
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < nd; j += gridDim.x * 256u) {
        const uint32_t i = a.fbl[j];
        const uint32_t e = a.ent[i];
        uint8_t *xg;
        uint8_t idx;
        Ctx c = make_ctx(a);
        elem_at(a, i, xg, idx, c);
        // (IL) k_local_fused wrote the op back whole, its patch applied: the key is the element's
        uint8_t *entry = IL ? entry_home<IL>(a, e, *reinterpret_cast<const uint64_t *>(xg)) : entry_of(a, e);
        Meta m;
        meta_load(entry, m);
        const uint32_t f = first_cand(*fw_of(a, ent_id<IL>(e)), a.rtag0);
        uint8_t st = kStDone;
        if (f == kNone || i < f) {
            Meta tm = m;
            dispatch<31>(kLocal, xg, entry, idx, tm, c);
            if (a.error_flags && !meta_equal(tm, m)) atomicOr(a.error_flags, 1u);
        } else if (i == f) {
            apply_to_shadow<kLocal, 31>(a, nullptr, i, entry);
            st = kStCommit;
        } else {
            const Meta m1 = after_first<kLocal>(a, m, f, 0);
            Meta tm = m1;
            dispatch<31>(kLocal, xg, entry, idx, tm, c);
            if (a.error_flags && !meta_equal(tm, m1)) atomicOr(a.error_flags, 1u);
        }
        a.st[i] = st;
        note_state(a, i, xg);
    }
}

// k_commit for 64-B entries over few commits (the local direct path: one per key a PUT first
// wrote): each wave takes 1024 elements, reads their stage bytes 16 per lane, lists the committing
// ones in LDS (a wave-wide prefix sum of the per-lane counts), then copies their shadows 16
// entries at a time, four lanes per entry. One wave per 1024 elements instead of one thread per
// element: k_commit's cost was its 4M threads, not its copies.
constexpr int kCwElems = 1024;
template <bool IL = false>
__global__ __launch_bounds__(256) void k_commit_w(BatchArgs a)
{
    __shared__ uint32_t lst[4][kCwElems];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t e0 = ((int64_t)blockIdx.x * 4 + w) * kCwElems + 16 * lane;
    uint32_t m = 0;
    if (e0 + 16 <= a.n) {   // st is 256-byte aligned and e0 a multiple of 16
        const uint4 s4 = *reinterpret_cast<const uint4 *>(a.st + e0);
        const uint32_t sw[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (((sw[b >> 2] >> (8 * (b & 3))) & 0xFFu) == kStCommit) m |= 1u << b;
    } else {
        for (int b = 0; b < 16; ++b)
            if (e0 + b < a.n && a.st[e0 + b] == kStCommit) m |= 1u << b;
    }
    const uint32_t c = __popc(m);
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += v;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    for (uint32_t pos = incl - c; m; m &= m - 1) lst[w][pos++] = (uint32_t)e0 + (uint32_t)(__ffs(m) - 1);
    __syncthreads();
    const int q = lane & 3;
    for (uint32_t j = (uint32_t)(lane >> 2); j < total; j += 16) {
        const uint32_t i = lst[w][j];
        const uint4 v = reinterpret_cast<const uint4 *>(shadow_of(a, i))[q];
        if (IL) {   // the shadow is an entry image: its key (bytes 8..15, lane 0's) names the bucket
            const uint64_t key = (uint64_t)(uint32_t)__shfl((int)v.z, 0, 4) | ((uint64_t)(uint32_t)__shfl((int)v.w, 0, 4) << 32);
            reinterpret_cast<uint4 *>(entry_home<IL>(a, a.ent[i], key))[q] = v;
        } else {
            reinterpret_cast<uint4 *>(entry_of(a, a.ent[i]))[q] = v;
        }
    }
}

// Separate inline instances of the local kernels: a runtime branch in k_local_fused cost a wave of occupancy
// 
template <bool IL>
static void launch_local_il(const BatchArgs &a, hipStream_t s)
{
    const int64_t n = a.n;
    const dim3 pgrid((unsigned)((n + kPreElems - 1) / kPreElems));
    const dim3 fgrid((unsigned)((n + 32 * kLfWaves - 1) / (32 * kLfWaves)));
    hipLaunchKernelGGL(k_local_pre<IL>, pgrid, dim3(kPreThreads), 0, s, a);
    hipLaunchKernelGGL(k_local_fused<IL>, fgrid, dim3(64 * kLfWaves), 0, s, a);
    // the waiting elements' count is on the device: enough workgroups for the rounds after a
    // membership change (configs[4]: ~100 K elements of keys a failed peer left INVALID), which
    // return at once when there are few
    hipLaunchKernelGGL(k_local_deferred<IL>, dim3(128u), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_commit_w<IL>, dim3((unsigned)((n + 4 * kCwElems - 1) / (4 * kCwElems))), dim3(256), 0, s, a);
}

int launch_local(const BatchArgs &a, const BatchPlan &p, hipStream_t s)
{
    if (p.il) launch_local_il<true>(a, s);
    else launch_local_il<false>(a, s);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace hkv
