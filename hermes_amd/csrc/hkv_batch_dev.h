// hkv_batch_dev.h -- what the batch path's translation units share (internal): the kernels' argument block
// (BatchArgs), the per-launch plan (BatchPlan, made by plan_batch in hkv_batch.hip), the launchers of the engines
// that have a file of their own, and the device helpers more than one file uses: the element, first-candidate
// (F word), shadow and lookup families. A helper of one file is in that file.
//   hkv_batch.hip        the plan, launch_batch, the rounds and unique-key engines and the partitioned host
//                        launches (each still to get its own file)
//   hkv_batch_small.hip  the single-workgroup engine, k_small
//   hkv_batch_local.hip  the direct local path: k_local_pre, k_local_fused, k_local_deferred, k_commit_w
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hkv_exec.h"
#include "hkv_internal.h"
#include "hkv_table_dev.h"

namespace hkv {

constexpr uint32_t kNone = 0xFFFFFFFFu;
// per-element stage between passes; kStCommit: the element's shadow holds its key's latest state
// (committed to the entry by k_commit unless a later round's first candidate supersedes it)
// kStDefer (the direct local path): the element waits for k_local_deferred
enum : uint8_t { kStDone = 0, kStCommit = 1, kStPend = 2, kStDefer = 3 };
enum { kCtrFbM = 1, kCtrFbL = 2, kCtrDefer = 3 };  // fallback: mem cursor, list length; local path: waiting elements

struct BatchArgs {
    uint8_t *elems;
    const int32_t *counts;
    const int32_t *offsets;      // packed INV/VAL launches (counts NULL, stride = n): batch offsets
    const uint8_t *index;
    uint8_t *log;
    uint8_t *rw;
    int32_t *ns_idx;
    unsigned long long *fw;      // [log_cap / 64] F word per 64-B log line (table-wide), see fw_index
    unsigned long long *fx, *fy; // [log_cap / 64] INV words X, Y (INV direct path; zero between launches)
    unsigned long long *ft;      // [log_cap / 64][8] ACK words T (ACK direct path; epoch << 32 | ~i)
    uint32_t fw_mask;
    uint32_t *ent;               // [n] entry id of every element (kNone: skipped or missing)
    uint8_t *st;                 // [n] stage (kSt*)
    uint32_t *pf;                // [n] pending element: its key's first candidate of the last round
    uint8_t *shadow;             // [cap][entry_size] entry image a round's first candidate produced
    unsigned long long *mem;     // [2 cap] fallback (F_R, element) pairs of workgroups with more than kFbLds
    uint32_t *fbl;               // [cap] fallback list: elements still pending after the last round
    uint32_t *ctr;               // kCtr*
    unsigned int *error_flags;
    Geometry g;
    int64_t n;
    int64_t rw_stride;
    int32_t stride;
    int32_t esz;
    int32_t type;
    uint32_t rtag0;              // round 0's tag; round r uses rtag0 + r
    uint8_t ltag;                // launch tag (1..255) in the seqlock byte of keys with a round-0 candidate
    int32_t rounds;              // rounds after round 0 before the fallback
    int32_t inv_direct;          // INV launch on the direct path (k_inv_resolve)
    int32_t ack_direct;          // ACK launch on the direct path (k_ack_resolve)
    uint8_t g_membership;
    uint8_t w_ack_init;
    int32_t *node_suspected;     // small launches write it themselves
    int32_t n_batches;
    const uint8_t *host_src;     // small launches staged in host memory (BatchLaunch)
    uint8_t *host_dst;
    uint8_t *dev_region;
    uint64_t region_bytes;
    uint32_t *done_flag;
    uint32_t done_value;
    unsigned long long *prof;    // HKV_SMALL_PROF: phase timestamps of k_small (debug)
    const SmallBatch *hdr;       // mixed small launches: the batch headers (in dev_region)
    uint8_t *state_out;          // local launches: each element's final state byte (may be NULL)
    const uint8_t *opc;          // local launches: the caller's opcode mirror (may be NULL, see k_local_pre)
    const uint8_t *patch;        // local direct path: pending header writes (hkv_batch_desc.d_patch), or NULL
    uint16_t *fk;                // local launches with RMWs: [n] each round-0 candidate's kind of mutation (fk_kind,
                                 // k_lookup), so k_resolve0_direct can resolve the elements after an absorbing F
    uint64_t *hx;                // big local launches with patches (patch_in_resolve): [2 n] each patched element's
                                 // header word (bytes 8..15) as patched and its op's last 8-byte word, from
                                 // k_lookup for k_resolve0_direct; NULL otherwise
    uint8_t *rws;                // ACK launches: read_write_ops state mirror (hkv_batch_desc.d_rw_state), or NULL
    const uint8_t *rwo;          // ACK launches: read_write_ops opcode mirror (hkv_batch_desc.d_opcode_in), or NULL
    int32_t n_rows, skip_row;    // HKV_BATCH_ROWS: rows applied in order (k_unique_rows), one skipped (-1: none)
    int64_t row_stride;          // elements between rows
    int32_t dbg;                 // HKV_DBG: timing experiments that skip work (results invalid); always 0
                                 // unless the library is built with -DHKV_DEBUG_MODES (HKV_DBG_ON)
    int32_t check_unique;        // HKV_CHECK_UNIQUE: HKV_BATCH_UNIQUE launches verify their keys are unique
    uint8_t *ack_out;            // INV launches: each element's ACK (hkv_batch_desc.d_ack_out), or NULL
    uint32_t ack_out_size;
    uint8_t *line;               // the inline residency (128 B per bucket), read and written by the <.., IL = true>
                                 // instances only; NULL for every other launch
};

// The engine that runs a launch. plan_batch (hkv_batch.hip) tests for them in this order; every engine is
// byte-exact against the oracle, so the choice shows only as time.
enum class Engine : uint8_t {
    kSmall,            // k_small: one workgroup, one kernel
    kLocalDirect,      // k_local_pre, k_local_fused, k_local_deferred, k_commit_w
    kRows,             // k_unique_rows (HKV_BATCH_ROWS)
    kUniqueLds64,      // k_unique_lds: 64-B entries and elements staged in LDS
    kUniqueLdsBig,     // k_unique_big: big-object INVs staged in LDS
    kUniqueInPlace,    // k_unique
    kValsOnePass,      // k_lookup alone
    kRoundsAckDirect,  // k_lookup, k_ack_resolve
    kRoundsInvDirect,  // k_lookup, k_inv_resolve, k_inv_commit
    kRoundsSlab,       // k_lookup, k_resolve0 on an LDS slab, rounds, k_commit, fallback
    kRoundsInPlace,    // k_lookup, k_resolve0_direct (big ops in place), rounds, k_commit, fallback
};
// How a launch's pending header writes (BatchLaunch::patch) are taken
enum class Patches : uint8_t {
    kNone,        // there are none
    kApplyFirst,  // k_apply_patch writes them into the ops, then the launch runs as usual
    kByEngine,    // the direct local path reads them beside the ops
    kInResolve,   // patch_in_resolve: k_lookup reads them, k_resolve0_direct writes the patched ops
};
// Patches::kInResolve records a patched value fill as a VCopy without a source (VCopy::fill), which only the wave's
// word copies know (wave_value_words_n; the byte-wise wave_value_copies_n would load through the null source). So
// the largest value plan_batch gives kInResolve must be one wave_value_copies still copies by words.
constexpr uint32_t kPirMaxValue = 320;
constexpr uint32_t kWaveWordsMaxValue = 8 * 62;   // nw + 1 <= 64 source words
static_assert(kPirMaxValue <= kWaveWordsMaxValue, "wave_value_copies_n ignores VCopy::fill: handle it there first");
struct BatchPlan {
    int refuse;            // 0, or the code launch_batch returns without launching anything
    Engine engine;
    Patches patches;
    int sv;                // value-size class the kernels are instantiated for: 31, 287, or 0 (any other)
    int rmax, ch;          // kRows: rows an instance holds (2 or 8), 16-B chunks of an element in LDS (1 or 4)
    int slab_threads;      // kRoundsSlab: threads (= elements) per k_resolve0 block
    int64_t lookup_head;   // rounds: elements of k_lookup's first launch (the whole launch unless it is split)
    bool big;              // ops of more than 64 B
    bool mixed;            // kSmall: a mixed launch (batch headers in the device region)
    bool inv_direct, ack_direct;   // BatchArgs::inv_direct / ack_direct
    bool ack_out;          // the launch writes ACKs (BatchArgs::ack_out set)
    bool state_out, opc;   // BatchArgs::state_out (local types) / opc (kLocal) take the caller's mirrors
    bool fk;               // BatchArgs::fk set: local launches with RMWs on big ops (k_resolve0_direct's)
    bool rw_mirrors;       // BatchArgs::rws / rwo set (ACK launches)
    bool node_suspected;   // k_node_suspected runs after the engine (INV launches; k_small writes it itself)
    bool il;               // the launch runs on the inline residency (BatchLaunch::line set)
    bool inline_instance;  // its engine has instances that know the inline residency
};

// Launchers of the engines outside hkv_batch.hip; each returns 0 or launch_batch's -3
int launch_small(const BatchArgs &a, const BatchPlan &p, hipStream_t s);   // Engine::kSmall (hkv_batch_small.hip)
int launch_local(const BatchArgs &a, const BatchPlan &p, hipStream_t s);   // kLocalDirect (hkv_batch_local.hip)

// f(std::integral_constant<...>) for a run-time selector, so a kernel family's launch line is written once
template <class F>
inline void with_sv(int sv, F &&f)
{
    if (sv == 31) f(std::integral_constant<int, 31>{});
    else if (sv == 287) f(std::integral_constant<int, 287>{});
    else f(std::integral_constant<int, 0>{});
}
template <class F>
inline void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

__device__ __forceinline__ Ctx make_ctx(const BatchArgs &a)
{
    Ctx c;
    c.g = a.g;
    c.g_membership = a.g_membership;
    c.w_ack_init = a.w_ack_init;
    c.rw = nullptr;
    c.rws = nullptr;
    c.rw_done = nullptr;
    c.vc = nullptr;
    return c;
}

__device__ __forceinline__ uint64_t phys_of(const BatchArgs &a, uint32_t e) { return (uint64_t)e * a.g.entry_unit; }
__device__ __forceinline__ uint8_t *entry_of(const BatchArgs &a, uint32_t e) { return a.log + phys_of(a, e); }

// 16 bytes at an 8-byte aligned address (op headers, log lines): one dwordx4 access
struct __attribute__((aligned(8))) U64x2 {
    uint64_t a, b;
};

// The state a key is in after any mutation by an element of this batch type, when that state
// makes every later element of the launch a non-mutating one whose result depends on the state
// alone (rounds_for == 0):
//   local, RMWs off: a mutation is a PUT (update_actions -> WRITE, hermesKV.c:100-141) or a GET
//     replay (-> REPLAY, :155-175); under either, GETs stall (:279-282) and PUTs stall (:352-354).
//   VALs: hermes_exec_val only ever sets VALID (:676-703) and its opcode is VAL_SUCCESS whatever
//     the state; under VALID no VAL mutates.
template <int TYPE>
__device__ __forceinline__ uint8_t absorbing_state()
{
    return TYPE == kVals ? kValid : kWrite;
}

// The meta every element after F (its key's only mutation in the launch) runs against, from S_0.
// Without the skew optimisations only the absorbing state matters. With them, a stalled GET or
// PUT also reads the timestamp and tells WRITE from REPLAY (hermesKV.c:196-238), so the meta is
// S_1 itself: after a PUT, update_actions' WRITE with version + 2 and this machine's cid
// (hermesKV.c:100-141, RMWs off); after a GET replay, REPLAY with the timestamp unchanged
// (:155-175). f_is_put: F is known to be a PUT (else its opcode is read).
template <int TYPE>
__device__ __forceinline__ Meta after_first(const BatchArgs &a, const Meta &m0, uint32_t f, int f_is_put)
{
    Meta m1 = m0;
    m_set_state(m1, absorbing_state<TYPE>());
    if (TYPE != kLocal || a.g.skew == 0) return m1;
    uint8_t foc = f_is_put ? (uint8_t)kOpPut : a.elems[(int64_t)f * a.esz + 8];
    if (a.hx && !f_is_put) {   // patch_in_resolve: F's op may not be patched yet (its patch is valid at byte 14)
        const uint64_t pb = *reinterpret_cast<const uint64_t *>(a.patch + (int64_t)f * 16 + 8);
        if ((pb >> 48) & 0xFFu) foc = (uint8_t)pb;
    }
    if (foc != kOpGet) {
        m1.ver += 2;
        m_set_cid(m1, (uint8_t)a.g.machine_id);
    } else {
        m_set_state(m1, kReplay);
    }
    return m1;
}

// The batch holding element i and its first element: i / stride, or for a packed launch the last
// batch whose offset is <= i (empty batches share their successor's offset)
__device__ __forceinline__ int32_t batch_of(const BatchArgs &a, int64_t i, int64_t &start)
{
    if (!a.offsets) {
        const int32_t b = (int32_t)(i / a.stride);
        start = (int64_t)b * a.stride;
        return b;
    }
    int lo = 0, hi = a.n_batches - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= i) lo = mid; else hi = mid - 1;
    }
    start = a.offsets[lo];
    return lo;
}

// batch_of's search for a whole wave (k_unique_rows): a 64-ary search over the n offsets that narrows
// [lo, hi] -- offsets[lo] <= i, the answer within -- until at most `span` batches follow lo, and returns lo.
// Each step samples lo + step, lo + 2 step, .. lo + 64 step (kary_sample); count(lo, hi) says how many of the
// samples at or below hi hold an offset <= i (a prefix: offsets ascend), which a wave answers with one coalesced
// load and a ballot and a host loop by looking. span 0 is batch_of itself; span 63 leaves the rest to a
// window of the offsets from lo on (rows_window_batch): two steps for up to 2^18 batches, against 18.
constexpr int kRowsWindow = 128;   // offsets lo .. lo + 127: the block's first batch is among the first 64
__host__ __device__ inline int32_t kary_stride(int32_t lo, int32_t hi) { return (hi - lo + 63) >> 6; }
// sample s (0 .. 63) of a step, and the range after c of the step's samples were in range and <= i
__host__ __device__ inline int32_t kary_sample(int32_t lo, int32_t hi, int s) { return lo + (s + 1) * kary_stride(lo, hi); }
__host__ __device__ inline void kary_narrow(int32_t &lo, int32_t &hi, int32_t c)
{
    const int32_t step = kary_stride(lo, hi);
    lo += c * step;
    if (lo + step - 1 < hi) hi = lo + step - 1;
}
template <class Count>
__host__ __device__ inline int32_t kary_last_le(int32_t n, int32_t span, Count &&count)
{
    int32_t lo = 0, hi = n - 1;
    while (hi - lo > span) kary_narrow(lo, hi, count(lo, hi));
    return lo;
}

// The batch of position i from the window win(k) = offsets[lo + k] (k < kRowsWindow; a k whose batch does not
// exist reads as INT32_MAX), scanned from k0 (win(k0) <= i, or k0 == 0): lo + the last k with win(k) <= i.
// The scan ends at the first offset above i_max >= i, so a wave that passes its last position's i_max runs it
// in step, k and win(k) the same in every lane. False when the window may end before i's batch (a run of
// empty batches): the caller asks batch_of.
template <class Win>
__host__ __device__ inline bool rows_window_batch(Win &&win, int32_t lo, int32_t k0, int64_t i, int64_t i_max, int32_t &b)
{
    int32_t k = k0;
    for (int32_t j = k0 + 1; j < kRowsWindow; ++j) {
        const int32_t v = win(j);
        if ((int64_t)v > i_max) break;
        if ((int64_t)v <= i) k = j;
    }
    b = lo + k;
    return k + 1 < kRowsWindow;
}

// The read_write_ops of batch b and its mirrors
__device__ __forceinline__ void batch_rw(const BatchArgs &a, int32_t b, Ctx &c)
{
    c.rw = a.rw ? a.rw + (int64_t)b * a.rw_stride : nullptr;
    c.rws = a.rws ? a.rws + (int64_t)b * (a.rw_stride / a.g.op_size) : nullptr;
    c.rwo = a.rwo ? a.rwo + (int64_t)b * (a.rw_stride / a.g.op_size) : nullptr;
}

__device__ __forceinline__ void elem_at(const BatchArgs &a, uint32_t i, uint8_t *&x, uint8_t &idx, Ctx &c)
{
    c.rw = nullptr;
    c.rws = nullptr;
    idx = 0;
    if (a.rw || !a.offsets) {  // packed INV / VAL elements need neither (exec_inv / exec_val)
        int64_t start;
        const int32_t b = batch_of(a, i, start);
        idx = (uint8_t)(i - start);
        batch_rw(a, b, c);
    }
    x = a.elems + (int64_t)i * a.esz;
}

// the state mirror of a local launch: written by whichever pass finishes the element
__device__ __forceinline__ void note_state(const BatchArgs &a, int64_t i, const uint8_t *x)
{
    if (a.state_out) a.state_out[i] = x[9];
}

// Live entries never overlap and are at least 64 B long, so their first 64-B lines are distinct.
// The F word of line l sits at l * odd mod 2^k (a bijection on the log's 2^k lines): keys that are
// neighbours in the log -- the hottest ids of a populated table are -- get F words on different
// lines, and memory-side atomics on one line serialise.
__device__ __forceinline__ uint32_t fw_index(const BatchArgs &a, uint64_t phys)
{
    return (uint32_t)(((phys >> 6) * 0x9E3779B1ull) & a.fw_mask);
}
__device__ __forceinline__ unsigned long long *fw_of(const BatchArgs &a, uint32_t e) { return a.fw + fw_index(a, phys_of(a, e)); }

__device__ __forceinline__ uint32_t first_cand(unsigned long long f, uint32_t rtag)
{
    return (uint32_t)(f >> 32) == ~rtag ? (uint32_t)f : kNone;
}

// F_r: atomicMin of ((~round tag) << 32 | element). The load filters most offers of a hot key:
// F only falls, and elements are dispatched roughly in element order.
__device__ __forceinline__ void offer(unsigned long long *f, uint32_t rtag, uint32_t i)
{
    const unsigned long long v = ((unsigned long long)(~rtag) << 32) | i;
    if (v < __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(f, v);
}

__device__ __forceinline__ uint8_t *shadow_of(const BatchArgs &a, uint32_t i)
{
    return a.shadow + (size_t)i * a.g.entry_size;
}

// entries and shadows are 8-byte aligned and a multiple of 8 long: 16-B words, then one 8-B word
__device__ __forceinline__ void copy_entry(uint8_t *dst, const uint8_t *src, uint32_t bytes)
{
    struct __attribute__((aligned(8))) W16 {
        uint64_t a, b;
    };
    uint32_t o = 0;
    for (; o + 16 <= bytes; o += 16) *reinterpret_cast<W16 *>(dst + o) = *reinterpret_cast<const W16 *>(src + o);
    if (o < bytes) *reinterpret_cast<uint64_t *>(dst + o) = *reinterpret_cast<const uint64_t *>(src + o);
}

// The round's first candidate of a key: S_r (read from src: the entry in round 0, the previous
// round's shadow later) -> S_{r+1}, written to the element's own shadow image, so the round's
// other elements, resolved concurrently, still read S_r. Later rounds read the shadow; the key's
// last shadow is committed to the entry once, by k_commit.
template <int TYPE, int SV>
__device__ __forceinline__ void apply_to_shadow(const BatchArgs &a, uint8_t *x, uint32_t i, const uint8_t *src)
{
    uint8_t *sh = shadow_of(a, i);
    Meta m;
    meta_load(src, m);
    if (SV == 31) {  // 64-B entries and shadows are 16-byte aligned
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(sh);
        const uint4 w0 = s4[0], w1 = s4[1], w2 = s4[2], w3 = s4[3];
        d4[0] = w0;
        d4[1] = w1;
        d4[2] = w2;
        d4[3] = w3;
    } else {
        copy_entry(sh, src, a.g.entry_size);
    }
    Ctx c = make_ctx(a);
    uint8_t *xg;
    uint8_t idx;
    elem_at(a, i, xg, idx, c);
    // x: the element's LDS copy (k_resolve0), or null: the element in global memory. Two calls,
    // not one on a select of the two, so each keeps its address space (no flat accesses).
    if (x) dispatch<SV>(TYPE, x, sh, idx, m, c);
    else dispatch<SV>(TYPE, xg, sh, idx, m, c);
    meta_store(sh, m);
}

// ---- pending header writes (hkv_batch_desc.d_patch, HKV_PATCH_BYTES per element): the second
// 8-B word of a patch holds opcode (bits 0..7), val_len (8..15), flags (16..31), the value fill
// byte (32..39), ts reset (40..47) and valid (48..55).
__device__ __forceinline__ bool patch_valid(uint64_t pb) { return ((pb >> 48) & 0xFFu) != 0; }

// element i lies inside its batch's count (launches are under 2^31 elements: 32-bit division,
// and none at all without counts)
__device__ __forceinline__ bool in_count(const BatchArgs &a, uint32_t i)
{
    if (!a.counts) return true;
    const uint32_t b = i / (uint32_t)a.stride;
    return (int32_t)(i - b * (uint32_t)a.stride) < a.counts[b];
}

// The key (bytes 8..15) and the meta (bytes 16..32) of a log line held 16 B per lane, in every lane
__device__ __forceinline__ uint64_t line_key_meta(const uint4 &ln, Meta &m)
{
    const uint64_t ek = (uint64_t)(uint32_t)__shfl((int)ln.z, 0, 4) | ((uint64_t)(uint32_t)__shfl((int)ln.w, 0, 4) << 32);
    m.w4 = (uint32_t)__shfl((int)ln.x, 1, 4);
    m.w5 = (uint32_t)__shfl((int)ln.y, 1, 4);
    m.ver = (uint32_t)__shfl((int)ln.z, 1, 4);
    const uint32_t w7 = (uint32_t)__shfl((int)ln.w, 1, 4);
    const uint32_t b32 = (uint32_t)__shfl((int)ln.x, 2, 4) & 0xFFu;
    m.llw_cid = (uint8_t)w7;
    m.llw_ver = (w7 >> 8) | (b32 << 24);
    return ek;
}

constexpr int kLookupPair = 2;
// Four lanes (q = lane & 3) look up kLookupPair keys side by side: the 64-B bucket (16 B per
// lane), the reference's slot order (first tag match, hermesKV.c:954-975), the log window
// (:969-970), then each lane's 16 B of the 64-B log line (bytes 16q..16q+15). All four lanes of a
// group call it with the same arguments.
// IL (the inline instances, a.line set): the bucket is the first half of its 128-B line and each lane loads its
// 16 B of the second half -- the inline key's entry -- in the same step; a hit on the flagged slot takes those
// bytes, any other hit loads the log line as before. home: where the hit's entry bytes live (writes go there);
// inl: the hit is its bucket's inline key. phys stays the log offset either way (the key's identity).
// beside: the caller's own work between the issue of the bucket loads and their first use (its loads ride
// along with them: k_unique_rows' batch search)
struct NothingBeside {
    __device__ __forceinline__ void operator()() const {}
};
template <int P = kLookupPair, bool IL = false, bool F = false, class Beside = NothingBeside>
__device__ __forceinline__ void lookup_core(const BatchArgs &a, const uint64_t *key, const bool *probe, int q,
                                            int gbase, bool *ok, uint64_t *phys, uint4 *ln, unsigned long long *fwv,
                                            uint8_t **home, bool *inl, Beside &&beside = Beside{})
{
    uint4 v[P], ev[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (IL) {
            const uint4 *l = line_words(a.line, bucket_of(a.g, key[k]));
            v[k] = probe[k] ? l[q] : make_uint4(0u, 0u, 0u, 0u);
            ev[k] = probe[k] ? l[4 + q] : make_uint4(0u, 0u, 0u, 0u);
        } else {
            v[k] = probe[k] ? bucket_words(a.index, bucket_of(a.g, key[k]))[q] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    beside();
    bool il[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        // group_probe (hkv_table_dev.h) with its tag test and slot mask written out: through slot_matches or
        // group_slots k_local_pre and k_unique_rows change their register counts (profiles/table_dev_registers.txt)
        const uint64_t s0 = u64_of(v[k].x, v[k].y), s1 = u64_of(v[k].z, v[k].w);
        const uint32_t tag = key_tag(key[k]);
        const bool mt0 = probe[k] && (s0 & 1u) && ((uint32_t)(s0 >> 1) & 0x7FFFFFu) == tag;
        const bool mt1 = probe[k] && (s1 & 1u) && ((uint32_t)(s1 >> 1) & 0x7FFFFFu) == tag;
        const uint32_t g0 = (uint32_t)(__ballot(mt0) >> gbase) & 0xFu;
        const uint32_t g1 = (uint32_t)(__ballot(mt1) >> gbase) & 0xFu;
        uint32_t o = 0;  // bit 2*l + j: slot 2*l + j matches
#pragma unroll
        for (int l = 0; l < 4; ++l) o |= ((g0 >> l) & 1u) << (2 * l) | ((g1 >> l) & 1u) << (2 * l + 1);
        const int first = o ? __ffs(o) - 1 : 0;
        const uint64_t raw = group_slot_word(slot_off_raw(s0), slot_off_raw(s1), first), off = off_of<IL>(raw);
        ok[k] = probe[k] && o && in_log_window(a.g, off);
        phys[k] = off & a.g.log_mask;
        il[k] = off_is_inline<IL>(raw) && ok[k];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (IL) {
            ln[k] = ev[k];
            if (!il[k]) ln[k] = ok[k] ? reinterpret_cast<const uint4 *>(a.log + phys[k])[q] : make_uint4(0u, 0u, 0u, 0u);
            if (home) home[k] = il[k] ? line_entry(a.line, a.g, key[k]) : a.log + phys[k];
            if (inl) inl[k] = il[k];
        } else {
            ln[k] = ok[k] ? reinterpret_cast<const uint4 *>(a.log + phys[k])[q] : make_uint4(0u, 0u, 0u, 0u);
            if (home) home[k] = a.log + phys[k];
            if (inl) inl[k] = false;
        }
        if (F) fwv[k] = ok[k] && q == 0 ? a.fw[fw_index(a, phys[k])] : ~0ull;
    }
}

template <int P = kLookupPair, bool IL = false>
__device__ __forceinline__ void lookup_pair(const BatchArgs &a, const uint64_t *key, const bool *probe, int q,
                                            int gbase, bool *ok, uint64_t *phys, uint4 *ln, uint8_t **home = nullptr,
                                            bool *inl = nullptr)
{
    lookup_core<P, IL, false>(a, key, probe, q, gbase, ok, phys, ln, nullptr, home, inl);
}

template <int P, bool IL, class Beside>
__device__ __forceinline__ void lookup_pair_beside(const BatchArgs &a, const uint64_t *key, const bool *probe, int q,
                                                   int gbase, bool *ok, uint64_t *phys, uint4 *ln, uint8_t **home,
                                                   Beside &&beside)
{
    lookup_core<P, IL, false>(a, key, probe, q, gbase, ok, phys, ln, nullptr, home, nullptr, beside);
}

// lookup_pair that also loads each hit's F word beside its log line (lane q == 0; ~0 for a miss), so a
// key's F costs no dependent load after the line (k_local_fused)
template <int P, bool IL = false>
__device__ __forceinline__ void lookup_pair_f(const BatchArgs &a, const uint64_t *key, const bool *probe, int q,
                                              int gbase, bool *ok, uint64_t *phys, uint4 *ln, unsigned long long *fwv,
                                              uint8_t **home = nullptr, bool *inl = nullptr)
{
    lookup_core<P, IL, true>(a, key, probe, q, gbase, ok, phys, ln, fwv, home, inl);
}

}  // namespace hkv
