// hkv_internal.h -- launch descriptors shared by the runtime and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hkv_codes.h"

struct hkv_table;

namespace hkv {

struct BatchLaunch {
    Geometry g;
    uint8_t *elems;
    const int32_t *counts;
    const int32_t *offsets;      // packed INV/VAL launches: n_batches + 1 batch offsets (counts NULL)
    uint8_t *state_out;          // local launches: each element's final state byte (may be NULL)
    const uint8_t *opcode_in;    // local launches: the caller's mirror of each element's opcode (may be NULL)
    const uint8_t *patch;        // local launches: pending header writes, 16 B per element (may be NULL)
    uint8_t *rw_state;           // ACK launches: state-byte mirror of read_write_ops (may be NULL)
    const uint8_t *index;
    uint8_t *log;
    uint8_t *line;               // the table's inline residency (hkv_runtime.hip "layouts"), or NULL: the launch
                                 // runs on index and log. Set only for launches batch_inline_capable() accepts
    uint8_t *rw;
    int64_t rw_stride;
    int32_t *ns_idx;
    int32_t *node_suspected;
    // round state (see hkv_batch.hip): F words per log line (table-wide, all-ones when
    // allocated) and per-launch scratch carved by batch_carve
    unsigned long long *fw;
    unsigned long long *fx, *fy;              // INV words per log line (zero between launches)
    unsigned long long *ft;                   // ACK words, eight per log line (tagged with the epoch)
    unsigned long long *mem;
    uint32_t *ent, *fbl, *pf, *ctr;
    uint64_t *hx;                // [2 cap] patched headers of big local launches (BatchArgs::hx)
    uint16_t *fk;                // [cap] round-0 candidates' kinds of mutation (BatchArgs::fk)
    uint8_t *st, *shadow;
    uint32_t cap;                             // elements the scratch was carved for
    uint32_t epoch;                           // launch counter of the table, 1..batch_max_epoch()
    unsigned int *error_flags;                // checked builds: unsound would_mutate()
    int64_t n;
    int32_t n_batches;
    int32_t stride;
    int32_t esz;
    int32_t type;
    uint8_t g_membership;
    uint8_t w_ack_init;
    int32_t path;                             // kPath*: which engine runs the launch
    int32_t unique;                           // HKV_BATCH_UNIQUE: no key twice in the launch
    int32_t n_rows, skip_row;                 // HKV_BATCH_ROWS (n_rows 0: a plain launch)
    uint8_t *ack_out;                         // INV launches: the ACK marshal's output (hkv_batch_desc.d_ack_out)
    uint32_t ack_out_size;
    int64_t row_stride;
    // small launches staged in host memory (the combining submit of hermes_batch_ops_to_KVS): the
    // kernel first copies region_bytes from host_src to dev_region (where elems, counts, rw and
    // node_suspected point), at the end copies them back to host_dst, then stores done_value into
    // *done_flag at system scope. region_bytes = 0: everything already in device memory.
    const uint8_t *host_src;
    uint8_t *host_dst;
    uint8_t *dev_region;
    uint64_t region_bytes;
    uint32_t *done_flag;
    uint32_t done_value;
    // mixed small launches (host-staged): n_batches headers at dev_region, batches of any type and
    // element size back to back; elems/counts/stride/esz/type/rw/node_suspected unused
    const struct SmallBatch *hdr;
};

// One batch of a mixed small launch; offsets are bytes from the launch's device region.
struct SmallBatch {
    int32_t type, count, esz, elem_off;
    int32_t rw_off, ns_off;   // -1: none (rw: ACK batches' read_write_ops; ns: INV batches' node_suspected)
    uint8_t g_membership, w_ack_init, pad0, pad1;
    int32_t pad2;
};
constexpr int kSmallMaxBatches = 64;

// ---- partitioned host launches (the combining submit of hermes_batch_ops_to_KVS, 64-B entries):
// every element goes to the workgroup that owns its key, part_of(key) of kPartG, so workgroups
// never share a key and need no communication. Each caller stages its own batch, partition-major
// (elements in element order within a partition), in its own pinned buffer; the launch carries one
// HostPartHdr per batch and part[g][b]: batch b's elements of partition g are
// [part[g][b], part[g + 1][b]) of its staged array -- all in the kernel arguments, which the
// dispatch delivers with the launch (no PCIe round trip for them).
constexpr int kPartG = 32;       // workgroups of one launch
constexpr int kPartCap = 256;    // elements one workgroup takes
constexpr int kPartMaxB = 16;    // batches one launch combines
__host__ __device__ inline uint32_t part_of(uint64_t key)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 59);   // kPartG = 32
}
struct HostPartHdr {
    uint64_t elems;   // device address: the staged elements, partition-major
    uint64_t pos;     // device address: u16 position in the batch of each staged element
    uint64_t rw;      // ACK batches: device address of the read_write_ops copy, else 0
    int32_t type, count, esz;
    uint8_t g_membership, w_ack_init, pad0, pad1;
    uint64_t out;     // device address the results go to (pinned), or 0: back into elems
    uint64_t rwo;     // ACK batches staged in device memory: each read_write_ops slot's opcode there, else 0
};
static_assert(sizeof(HostPartHdr) == 56, "HostPartHdr is seven 8-byte words");
struct HostPartCommon {
    Geometry g;
    const uint8_t *index;
    uint8_t *log;
    unsigned int *error_flags;
    uint32_t *flags;             // device address: kPartG words, workgroup g stores seq into flags[g]
    unsigned long long *prof;    // HKV_PART_PROF: workgroup 0's phase timestamps (debug), or NULL
};
struct HostPartLaunch {          // one launch, everything in the kernel arguments
    HostPartCommon c;
    uint32_t seq;
    int32_t n_batches;
    HostPartHdr hdr[kPartMaxB];
    uint16_t part[kPartG + 1][kPartMaxB];
};
// one launch published to the serving kernel (pinned ring slot; seq written last)
struct alignas(128) HostRingSlot {
    uint32_t seq;
    int32_t n_batches;
    uint32_t pad[2];
    HostPartHdr hdr[kPartMaxB];
    uint16_t part[kPartG + 1][kPartMaxB];
};
struct HostServeLaunch {
    HostPartCommon c;
    const HostRingSlot *ring;    // device address of ring_n slots (pinned); launch n in slot n % ring_n
    int32_t ring_n;
    uint32_t epoch;
    const uint32_t *stop;        // pinned: non-zero makes every workgroup leave between launches
    uint32_t *exited;            // pinned: workgroup g stores epoch into exited[g] when it leaves
    uint64_t idle_ticks, life_ticks;   // wall_clock64 ticks (100 MHz)
    int32_t merge;               // launches one workgroup pass may take together (HKV_SERVE_MERGE; 1: one at a time)
    uint32_t start[kPartG];      // the first launch each workgroup takes
    int32_t spec;                // the first launch's headers read beside the merge scan (HKV_SERVE_SPEC)
};
int launch_host_serve(const HostServeLaunch &sl, hipStream_t s);
int launch_host_part(const HostPartLaunch &pl, hipStream_t s);

enum : int32_t { kPathAuto = 0, kPathEngine = 1, kPathSmall = 2 };

struct PopulateLaunch {
    uint64_t *first, *second;
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b;
    void *sort_tmp;
    size_t sort_tmp_bytes;
    uint8_t *index;
    uint8_t *log;
    unsigned long long *evictions;
    int64_t n;
    uint64_t bkt_mask;
    uint64_t log_cap, log_mask;
    uint64_t h0, k, hw;
    uint32_t entry_size;
    int32_t key_bits;
    uint8_t val_len_byte;
};

// A table's HBM image and geometry, for the workload kernels that read it (virtual peers take
// each key's current timestamp when they write it, hkv_workload.hip)
struct TableView {
    Geometry g;
    const uint8_t *index;
    const uint8_t *log;
    const uint8_t *line;   // non-NULL: the table is INLINE and the kernel reads the inline keys' entries there
};
// What a consumer of the view does with the table, which decides the layout it is given (hkv_runtime.hip
// "layouts"): kViewLog -- it reads index and log as they are (the table is converted to LOG first, on
// stream); kViewLive -- its kernels know the inline residency (the table goes to its preferred layout, as
// before an inline-capable batch launch); kViewStatic -- it reads only what never changes under the rounds
// (geometry, buckets, the keys of entries): no conversion.
enum : int32_t { kViewLog = 0, kViewLive = 1, kViewStatic = 2 };
int table_view(hkv_table *t, TableView *out, hipStream_t stream, int32_t mode);

// The private inline residency: one 128-B line per bucket -- the bucket, then the whole entry of
// the key in its lowest in-use slot, whose slot carries kInlineSlotBit. A located offset (k_peer_locate) and
// an entry id of a local launch's scratch carry the same fact in a spare bit.
constexpr uint64_t kInlineSlotBit = 1ull << 63;   // bit 39 of a slot's 40-bit offset field
constexpr uint64_t kInlineOffBit = 1ull << 39;    // ... as seen in the offset (slot >> 24)
constexpr uint64_t kInlineMaxLog = 1ull << 36;    // log_cap of an eligible table: offsets stay below bit 39,
                                                  // entry ids below bit 31
constexpr uint64_t kPhysInline = 1ull << 62;      // hkv_wl_peer_locate's offsets (~0: a miss)
// index + log -> lines (to_inline), or the inline entries back to their log offsets
int launch_layout_convert(const uint8_t *index, uint8_t *log, uint8_t *line, uint64_t num_bkts, uint64_t log_mask,
                          bool to_inline, hipStream_t s);
// The table census (hermeskv.h "Table census and digest"): one pass over the buckets -- of `line` when it is
// non-NULL (the table is INLINE), else of `index` -- into out[0 .. kCensusWords), which the launch zeroes first.
// offender_keys (may be NULL) takes up to offender_cap keys of live keys that are not VALID.
constexpr int kCensusWords = 25;   // sizeof(hkv_census) / 8
int launch_table_census(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                        uint64_t num_bkts, unsigned long long *out, unsigned long long *offender_keys,
                        uint64_t offender_cap, int device, hipStream_t s);
// The partitioned census (hermeskv.h "Partitioned census and delta repair"): the census's pass into
// rows[p][0..3] = {digest_sum, digest_xor, keys, not VALID} of the live keys with key & (2^part_bits - 1) == p,
// 2^part_bits <= num_bkts; overwritten (zeroed by the launch where its kernel adds to them). The rows' diff:
// mask[p] = rows a and b differ in any word (accumulate: or-ed into mask[p]), *count = non-zero bytes of mask.
int launch_table_census_parts(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                              uint64_t num_bkts, uint32_t part_bits, unsigned long long *rows, int device, hipStream_t s);
int launch_part_rows_diff(const void *a, const void *b, uint32_t part_bits, uint8_t *mask, unsigned long long *count,
                          int accumulate, int device, hipStream_t s);
// Replica repair (hermeskv.h "Replica repair"). Extract: one pass like the census over the buckets [bkt_lo, bkt_hi)
// -- of `line` when it is non-NULL, else of `index` -- that writes the masked entry image of every live slot whose
// timestamp is at least min_ts to records (compacted, at most record_cap of them) and counts into
// result[0] (records) and result[1] (scanned keys), which the launch zeroes first. part_sel (may be NULL: every
// bucket): 2^part_bits bytes; a bucket b with part_sel[b & (2^part_bits - 1)] == 0 is neither loaded nor counted.
int launch_table_extract(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                         uint64_t bkt_lo, uint64_t bkt_hi, uint64_t min_ts, uint8_t *records, uint64_t record_cap,
                         unsigned long long *result, const uint8_t *part_sel, uint32_t part_bits, int device,
                         hipStream_t s);
// Install: n records, no key twice, applied as an INV and (source VALID) a VAL each to the entries of `log`, or,
// with `line` non-NULL, to the lines for the inline keys; result[0..3] (raised, equal, older, missed) zeroed first.
// missed_flag (may be NULL: the install itself): one byte per record, 1 when the record was missed, else 0;
// 16-byte aligned and n rounded up to 64 bytes long (a wave stores its 16 records' bytes at once, zero past n).
int launch_table_install(const Geometry &g, const uint8_t *index, uint8_t *log, uint8_t *line, const uint8_t *records,
                         uint64_t n, unsigned long long *result, hipStream_t s, uint8_t *missed_flag = nullptr);
// Key-level delta repair (hermeskv.h "Key-level delta repair"), three read-only passes with the residency rule of
// the ones above (`line` non-NULL: the inline keys are read from their lines). Summaries: launch_table_extract's
// arguments and counts, with 16-B summaries (at most cap) where it writes records. Need: n summaries looked up and
// classed into result[0..5] (missed, newer, validate, same, state_only, older), the keys of the first three classes
// compacted to need_keys (at most need_cap) and counted in result[6]; result[0..7] zeroed first. Fetch: record i =
// the masked entry image of keys[i], or zero but for the key; result[0..1] (found, absent) zeroed first.
int launch_table_summaries(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                           uint64_t bkt_lo, uint64_t bkt_hi, uint64_t min_ts, uint8_t *summaries, uint64_t cap,
                           unsigned long long *result, const uint8_t *part_sel, uint32_t part_bits, int device,
                           hipStream_t s);
int launch_table_need(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                      const uint8_t *summaries, uint64_t n, unsigned long long *need_keys, uint64_t need_cap,
                      unsigned long long *result, int device, hipStream_t s);
int launch_table_fetch(const Geometry &g, const uint8_t *index, const uint8_t *log, const uint8_t *line,
                       const unsigned long long *keys, uint64_t n, uint8_t *records, unsigned long long *result,
                       int device, hipStream_t s);
// Sketch-level delta repair (hermeskv.h "Sketch-level delta repair", hkv_sketch.hip). Fold: n summaries into the
// 3 S cells, zeroed first unless accumulate. Decode: a -= b, the passes and the closing count, all enqueued at once;
// result[0..7] (hkv_sketch_result) zeroed first. api_fail: hkv_last_error()'s message for entry points outside
// hkv_runtime.hip; returns code.
int launch_sketch_fold(const uint8_t *summaries, uint64_t n, void *cells, uint64_t S, int accumulate, int device,
                       hipStream_t s);
int launch_sketch_decode(void *a, const void *b, uint64_t S, uint8_t *only_a, uint64_t cap_a, uint8_t *only_b,
                         uint64_t cap_b, unsigned long long *result, int device, hipStream_t s);
int api_fail(int code, const char *msg);
// The upsert's inserts (hermeskv.h "Upsert", step 2) into index and log, after an install with missed_flag and the
// host's read of its missed count m (1 <= m <= n <= 2^31 - 1): the scan of the flags into ranks, the missed
// records' (bucket, rank) pairs, their stable sort by bucket, the per-bucket replay of mica_insert_one, and the
// log entries. g.log_head is not read: h0, k, hw are plan_log's for m inserts from the table's head (h0 a multiple
// of 16). Scratch, all device memory: flags [n], ranks [n], scan_tmp; keys_a/b, vals_a/b, rec_of [m] 32-bit each,
// key_of [m] 64-bit, sort_tmp. counts[0] += replaced, counts[1] += evictions (the caller zeroes them); evictions:
// the table's counter. phase_events (may be NULL): four events, recorded after the scan and the pairs, the sort,
// the replay and the log writes.
struct UpsertLaunch {
    Geometry g;
    uint8_t *index, *log;
    const uint8_t *records;
    uint64_t n, m;
    const uint8_t *flags;
    uint32_t *ranks;
    void *scan_tmp;
    size_t scan_tmp_bytes;
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b, *rec_of;
    uint64_t *key_of;
    void *sort_tmp;
    size_t sort_tmp_bytes;
    unsigned long long *evictions, *counts;
    uint64_t h0, k, hw;
    int32_t key_bits;
    uint8_t val_len_byte;
    hipEvent_t *phase_events;
};
size_t scan_temp_bytes(uint64_t n);
int launch_upsert_inserts(const UpsertLaunch &u, hipStream_t s);
// whether launch_batch runs this launch on kernels that know the inline residency (bl.line aside)
bool batch_inline_capable(const BatchLaunch &bl);

constexpr int64_t kSmallMaxElems = 4096;   // launches the single-workgroup kernel can take
int launch_batch(BatchLaunch &bl, hipStream_t s);
int launch_populate(const PopulateLaunch &pl, hipStream_t s);
int launch_hash_ids(const uint32_t *ids, uint64_t *out, int64_t n, hipStream_t s);
size_t sort_temp_bytes(int64_t n, int key_bits);
// batch scratch for launches of up to cap elements (size, carving into bl); the table-wide F
// words (one per 64-B log line, all-ones when allocated and whenever the epoch wraps)
size_t batch_scratch_bytes(int64_t cap, uint32_t entry_size);
void batch_carve(BatchLaunch &bl, uint8_t *base, int64_t cap, uint32_t entry_size);
size_t batch_fw_words(uint64_t log_cap);
uint32_t batch_max_epoch();

}  // namespace hkv
