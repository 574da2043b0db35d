// hkv_batch_dev.h -- what the batch path's translation units share (internal): the kernels' argument block
// (BatchArgs), the per-launch plan (BatchPlan, made by plan_batch in hkv_batch.hip), and the few device helpers
// both use.
//   hkv_batch.hip        the plan, launch_batch, and the multi-kernel engines (rounds, direct local, unique),
//                        which share the lookup and shadow helpers defined there
//   hkv_batch_small.hip  the single-workgroup engine, k_small
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
enum : uint8_t { kStDone = 0, kStCommit = 1, kStPend = 2 };
enum { kCtrFbM = 1, kCtrFbL = 2 };  // fallback: mem cursor, list length

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

// Engine::kSmall's launcher (hkv_batch_small.hip); returns 0 or launch_batch's -3
int launch_small(const BatchArgs &a, const BatchPlan &p, hipStream_t s);

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

}  // namespace hkv
