/*
 * hermeskv.h -- C ABI of libhermeskv.so, the MI355X-native HermesKV data path.
 *
 * Drop-in boundary: the three entry points the reference's worker links
 * against, with the reference's exact signatures and argument meaning:
 *
 *   hermes_batch_ops_to_KVS   replaces include/hermes/spacetime.h:228-230 (hermesKV.c:905-996)
 *   spacetime_init            replaces include/hermes/spacetime.h:211     (spacetime.c:25-30)
 *   spacetime_populate_fixed_len replaces include/hermes/spacetime.h:212  (spacetime.c:32-68)
 *
 * The MICA-herd index and log (mica.h:62-91) live in HBM; op arrays are caller-owned host
 * memory, mutated in place exactly as the reference mutates them. Errors the reference turns
 * into asserts make these three calls print a message and abort (fail loudly); the hkv_* calls
 * return a negative code instead and leave a message in hkv_last_error().
 *
 * The hkv_* extensions are the device-resident fast path: tables created explicitly,
 * op arrays already in HBM, many batches (one per virtual worker) concatenated into one
 * launch, asynchronous on a caller-supplied HIP stream. Their results are defined as the
 * reference applied to the batches one after another (concatenation order).
 *
 * Plain pointers and sizes only; no HIP or torch types appear in any signature
 * (streams are passed as void* and interpreted as hipStream_t; NULL is the HIP null stream).
 */
#ifndef HERMESKV_H
#define HERMESKV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HKV_ABI_VERSION 10

/* ------------------------------------------------------------------ reference types
 * Declared here only when the reference's own spacetime.h has not been included; the
 * layouts are the reference's (gcc, x86-64): see hermes_amd/layout.py for every offset. */
#ifndef HERMES_SPACETIME_H
enum hermes_batch_type_t {               /* spacetime.h:219-226 */
    local_ops,
    local_ops_after_membership_change,
    invs,
    acks,
    vals
};
typedef struct { uint8_t bit_array[1]; } bit_vector_t;               /* bit_vector.h:40-44 */
typedef struct { uint8_t lock; uint32_t version; } __attribute__((packed)) seqlock_t;
typedef struct {                          /* spacetime.h:188-195, 8 bytes, passed by value */
    volatile uint8_t num_of_alive_remotes;
    volatile bit_vector_t g_membership;
    volatile bit_vector_t w_ack_init;
    seqlock_t lock;
} spacetime_group_membership;
typedef struct hkv_spacetime_op spacetime_op_t; /* 56-byte spacetime_op_t, used by pointer */
struct spacetime_kv;                            /* opaque; only its address is passed */
#endif

/* ------------------------------------------------------------------ reference entry points */

/* spacetime.h:228-230. op_array holds op_num elements of sizeof_op_elem bytes (56 for local
 * ops and INVs, 16 for ACKs/VALs, 56 for ACKs in an RMW build). read_write_ops is the
 * caller's local-op buffer (hkv_config.rw_len elements), written by ACK completions.
 * node_suspected is written by INV batches that carry ST_OP_MEMBERSHIP_CHANGE. thread_id is
 * accepted for signature compatibility (the reference uses it for debug prints only). */
#ifndef HKV_IMPLEMENTATION
void hermes_batch_ops_to_KVS(enum hermes_batch_type_t type, uint8_t *op_array, int op_num,
                             uint16_t sizeof_op_elem, spacetime_group_membership curr_membership,
                             int *node_suspected, spacetime_op_t *read_write_ops, uint8_t thread_id);
#endif
/* ABI note: the reference's callers are built by gcc, which passes the 8-byte (packed)
 * spacetime_group_membership in one general-purpose register. clang classifies the same
 * packed struct as MEMORY (stack), so the library defines this entry point with the 8 bytes
 * received as a uint64_t (HKV_IMPLEMENTATION), matching what gcc-built callers pass. */

/* spacetime.h:211. Creates the default table in HBM (hkv_set_default_config, else the
 * reference defaults: 2^21 buckets, 1 GiB log) and populates hkv_config.num_keys keys
 * (default 1,000,000) exactly as the reference does. instance_id becomes machine_id unless
 * hkv_set_default_config set one. */
void spacetime_init(int instance_id);

/* spacetime.h:212. Populates the default table (creating it if needed); kv is accepted for
 * signature compatibility and may be &kv or NULL. */
void spacetime_populate_fixed_len(struct spacetime_kv *kv, int n, int val_len);

/* ------------------------------------------------------------------ hkv extensions */

typedef struct hkv_config {
    uint32_t abi_version;       /* HKV_ABI_VERSION */
    uint32_t machine_id;        /* reference global machine_id (hrd.h:87) */
    uint32_t rmw_enabled;       /* ENABLE_RMWs (config.h:37) */
    uint32_t big_objects;       /* USE_BIG_OBJECTS (hrd.h:36) */
    uint32_t extra_cache_lines; /* EXTRA_CACHE_LINES (hrd.h:37). With big_objects: 1..16 accepted (values of
                                   31 + 64 c bytes in entries of 64 + 64 c: 95 B / 128 B up to 1055 B / 1088 B);
                                   anything else is refused by hkv_table_create. Without: ignored. The test suite
                                   holds c = 1, 2, 4, 5, 8 and 16 to the reference byte for byte, on every batch
                                   type and on census, extract and install (and c = 7 in the workload round). Only
                                   c = 4 (287-B values, the reference's configs[2]) has kernel instances of its
                                   own; every other c runs the general instances, correct at any accepted size,
                                   with no speed claim made for them */
    int32_t  device;            /* HIP device ordinal */
    uint32_t rw_len;            /* elements of read_write_ops (max_batch_size, default 250) */
    uint32_t skew_flags;        /* HKV_SKEW_*: the reference's opt-in skew optimisations (0 = off,
                                   the reference's default configuration) */
    uint64_t num_keys;          /* SPACETIME_NUM_KEYS (spacetime.h:21) */
    uint64_t num_bkts;          /* SPACETIME_NUM_BKTS (spacetime.h:22), power of two <= 2^31 */
    uint64_t log_cap;           /* SPACETIME_LOG_CAP (spacetime.h:23), power of two */
} hkv_config;

/* hkv_config.skew_flags: the exec-side skew optimisations of config.h:77-80, compile-time
 * switches in the reference and per table here. Both change only the op, never the key's meta.
 *   HKV_SKEW_READ_COMPLETE   ENABLE_READ_COMPLETE_AFTER_VAL_RECV_OF_HOT_REQS (config.h:79,
 *       hermesKV.c:224-238): a stalled GET records the key's timestamp the first time (its ts is
 *       (0, 0) after a refill) and completes, without copying a value, once the key's version is
 *       at least two above it (a write completed after the read was issued).
 *   HKV_SKEW_WRITE_COALESCE  ENABLE_WRITE_COALESCE_TO_THE_SAME_KEY_IN_SAME_NODE (config.h:80,
 *       hermesKV.c:196-221): a PUT stalling behind a local write records the key's version (16
 *       bits) when its own ts.version is 0, and completes (PUT_COMPLETE, no INV) once the key's
 *       version is at least two above it.
 * The refill-side flag (ENABLE_COALESCE_OF_HOT_REQS) is hkv_wl_refill's. */
#define HKV_SKEW_READ_COMPLETE  1u
#define HKV_SKEW_WRITE_COALESCE 2u

typedef struct hkv_table hkv_table;

/* One batch launch: n_batches batches of the same type, batch b owning elements
 * [b*stride, b*stride + counts[b]) of d_elems (HKV_BATCH_PACKED: see below), applied in
 * concatenation order. */
typedef struct hkv_batch_desc {
    int32_t  type;              /* enum hermes_batch_type_t */
    int32_t  n_batches;
    int32_t  stride;            /* elements reserved per batch */
    uint16_t elem_size;         /* sizeof_op_elem */
    uint16_t flags;             /* HKV_BATCH_*: which engine runs the launch (0 = by size) */
    uint8_t *d_elems;           /* device */
    const int32_t *d_counts;    /* device, n_batches entries; NULL = stride each */
    uint8_t *d_rw;              /* device base of batch 0's read_write_ops (ACK batches) */
    int64_t  rw_stride_bytes;   /* bytes between consecutive batches' read_write_ops */
    int32_t *d_node_suspected;  /* device, n_batches entries (INV batches); NULL = ignore */
    uint8_t  membership[8];     /* spacetime_group_membership by value */
    uint8_t *d_state_out;       /* device, local batches: receives each element's final state byte
                                   (op byte 9; n_batches * stride bytes), a mirror the worker loop's
                                   next passes can read instead of the ops; NULL = none (ABI 2) */
    const uint8_t *d_opcode_in; /* device, local batches: the caller's mirror of each element's opcode
                                   (op byte 8; n_batches * stride bytes), e.g. written by its refill
                                   (hkv_wl_refill); lets the launch find its PUTs without reading
                                   every op. A PUT the mirror misses raises error flag bit 3.
                                   NULL = read the ops (ABI 3). ACK batches with d_rw: the mirror of
                                   each read_write_ops slot's opcode (rw_stride_bytes / op size per
                                   batch), which a completion reads instead of the op; it must describe
                                   the ops (round 4) */
    const uint8_t *d_patch;     /* device, local batches: pending header writes, HKV_PATCH_BYTES per element
                                   (n_batches * stride), NULL = none (ABI 5). An element whose patch is
                                   valid first gets the patch's bytes, exactly as if the caller had written
                                   them into the op before the launch; hkv_wl_refill_plan writes a refill
                                   this way, so the launch's own write-back of every op replaces the
                                   refill's pass over the op slab. The mirrors (d_opcode_in) must already
                                   describe the patched ops. */
    uint8_t *d_rw_state;        /* device, ACK batches: a mirror of the read_write_ops' state bytes
                                   (rw_stride_bytes / op size per batch); every completion a launch writes
                                   into read_write_ops is also written here. NULL = none (ABI 5) */
    const uint64_t *d_put_keys; /* reserved, must be NULL (ABI 8; ABI 6-7: a PUT-key mirror for the local
                                   launch's prepass, measured slower and removed) */
    int32_t  n_rows;            /* HKV_BATCH_ROWS: rows of elements, applied row after row (ABI 6) */
    int32_t  skip_row;          /* HKV_BATCH_ROWS: a row that is not applied (-1: none) */
    int64_t  row_stride;        /* HKV_BATCH_ROWS: elements from one row to the next in d_elems */
    uint8_t *d_ack_out;         /* INV launches with HKV_BATCH_UNIQUE, 64-byte entries: element i's answer, as the
                                   worker's ACK callbacks make it (hermes_worker.c:69-118: an ACK from this
                                   machine for INV_SUCCESS, the element itself as INV-abort when ack_out_size holds
                                   it, else opcode ST_EMPTY), written to d_ack_out + i * ack_out_size by the launch
                                   itself, and each answered element leaves with opcode ST_EMPTY, as after the
                                   callbacks' send (ack_modify_elem_after_send). NULL = none (ABI 6)
                                   ACK launches with HKV_BATCH_ROWS, 16-byte ACKs and 64-byte entries: the VAL
                                   callbacks (hermes_worker.c:122-157) instead -- every row element of a batch
                                   whose result opcode is not ACK_SUCCESS, MEMBERSHIP_CHANGE or EMPTY is copied
                                   to d_ack_out + (r * row_stride + j) * 16 with opcode ST_OP_VAL and sender =
                                   this machine (val_copy_and_modify_elem), every other live position there
                                   gets opcode ST_EMPTY, and every non-empty element leaves with opcode
                                   ST_EMPTY (val_skip_or_get_sender_id, val_modify_elem_after_send);
                                   ack_out_size 16. Live positions are those of a batch's range in a row other
                                   than skip_row: the positions of skip_row and those past the last batch's
                                   end are not written (they keep what the buffer held), so a caller reads
                                   only live positions */
    uint32_t ack_out_size;
    const uint64_t *d_phys;     /* reserved, must be NULL (ABI 8; ABI 7: located entries that skipped the
                                   bucket read the reference makes, never the default, removed) */
} hkv_batch_desc;

/* d_patch layout (16 bytes per element): key 0..7, opcode 8, val_len 9, flags (RMW_flag | no_coales
 * << 1) 10..11, value fill byte 12 (0: the value is kept), ts reset 13 (1: ts bytes 11..15 := 0),
 * valid 14 (1: apply), 15 unused. Applying sets op bytes 0..7 = key, 8 = opcode, 9 = ST_NEW,
 * 10 = val_len, [11..15 = 0], 16..17 = flags and, with a fill byte, the ST_VALUE_SIZE value bytes. */
#define HKV_PATCH_BYTES 16

/* hkv_batch_desc.flags. By default launches of at most 4096 elements run as one single-workgroup
 * kernel and larger ones on the multi-kernel engine; both give the same bytes. */
#define HKV_BATCH_ENGINE 1u     /* always the multi-kernel engine */
#define HKV_BATCH_SMALL  2u     /* the single-workgroup kernel (launches of at most 4096 elements) */
/* INV, ACK and VAL batches stored back to back: d_counts holds n_batches + 1 element offsets (batch
 * b is elements [d_counts[b], d_counts[b+1]) of d_elems) and stride is the total, d_counts[n_batches];
 * an ACK batch b still completes into d_rw + b * rw_stride_bytes. Same results as the row layout;
 * no empty slots to launch over. */
#define HKV_BATCH_PACKED 4u
/* The caller guarantees that no key appears twice among the launch's elements (INV and ACK
 * launches): each element is then its key's only one and is applied to the entry in a single pass,
 * in any order. A replica's INV slab of one round has this property (a coordinator has at most one
 * write in flight per key: hermes_exec_write stalls while op_buffer_index is set,
 * hermesKV.c:331-344), and so have one peer's ACKs to it, so a receiver applies each peer's slab as
 * one such launch. A duplicate breaks the results; with HKV_CHECK_UNIQUE=1 in the environment every
 * launch checks and raises error flag bit 4. */
#define HKV_BATCH_UNIQUE 8u
/* With HKV_BATCH_UNIQUE, INV and ACK launches of 64-byte entries: n_rows (at most 8) launches of one
 * layout in one, applied in row order -- row r is the launch whose elements start at element
 * r * row_stride of d_elems (the same n_batches, stride, counts or offsets and read_write_ops for every
 * row), row skip_row excepted. Element j of every row carries the same key, or is a hole (opcode byte
 * 0: not an element of its row's batch; nothing of it is read or written). So each key is looked up
 * once and its elements applied one row after the other: a coordinator's ACKs from all its peers, lined
 * up with the INVs they answer, go in one launch, and so do INVs that peers sent for the same keys.
 * An element whose key differs from its position's raises error flag bit 4. d_node_suspected must be
 * NULL. */
#define HKV_BATCH_ROWS 16u   /* packed rows: elements past d_counts[n_batches] (<= stride) are in no batch */
/* Bits 5..7 are reserved (ABI 8; ABI 6-7: a local launch in two calls, HKV_BATCH_PREPASS / PREPASSED /
 * PREPASS_CANCEL, measured slower and removed): a launch that sets them fails. */
#define HKV_BATCH_RESERVED_FLAGS 0xE0u
#define HKV_MAX_ROWS 8
int  hkv_abi_version(void);
/* 1 when the library was built with work-skipping timing modes (-DHKV_DEBUG_MODES, HKV_DBG):
 * such a build is for timing experiments only and bench.py refuses to report from it. */
int  hkv_debug_modes(void);
const char *hkv_last_error(void);

int  hkv_table_create(const hkv_config *cfg, hkv_table **out);
int  hkv_table_destroy(hkv_table *t);
/* spacetime_populate_fixed_len on the device (reverse id order, MICA slot rules) */
int  hkv_table_populate(hkv_table *t, int64_t n, int val_len);
int  hkv_table_config(const hkv_table *t, hkv_config *out);
/* changes hkv_config.skew_flags of a table between launches (e.g. to time several policies on
 * one table); ordered after the launches already enqueued on the table's streams by the caller */
int  hkv_table_set_skew(hkv_table *t, uint32_t skew_flags);

/* device-resident batch path, asynchronous on `stream` (NULL = the HIP null stream). One
 * stream at a time per table: launches share the table's round scratch (entry ids, stages,
 * shadow images) and its per-log-line F/X/Y/T words. */
int  hkv_batch_async(hkv_table *t, const hkv_batch_desc *desc, void *stream);
int  hkv_sync(hkv_table *t, void *stream);

/* parity / debugging views of the HBM image (reference byte layout) */
int  hkv_copy_index(hkv_table *t, void *host_dst, uint64_t offset, uint64_t bytes);
int  hkv_copy_log(hkv_table *t, void *host_dst, uint64_t offset, uint64_t bytes);
uint64_t hkv_log_head(const hkv_table *t);
int64_t  hkv_num_index_evictions(const hkv_table *t);
void *hkv_device_index(hkv_table *t);
/* internal-consistency flags raised by the device path since the last call (0 = none);
 * bit 0: an element resolved in parallel (not a key's first mutating element) changed the meta;
 * bit 1: the ACK direct path completed a write from an unexpected state;
 * bit 2: a local launch's mutating element had not offered itself in its prepass;
 * bit 3: d_opcode_in missed a PUT;
 * bit 4: an HKV_BATCH_UNIQUE launch held a key twice (checked with HKV_CHECK_UNIQUE=1), or an
 *        HKV_BATCH_ROWS position's rows disagree on the key */
int  hkv_take_error_flags(hkv_table *t, uint32_t *out);
void *hkv_device_log(hkv_table *t);

/* Table layouts (ABI 9). The table image every export above returns is the reference's: a 64-B bucket per
 * index slot group and the log. The library may keep a second, private residency beside it, "inline": one
 * 128-B line per bucket holding the bucket and the whole 64-B entry of the key in its lowest in-use slot, so
 * that a lookup of that key (about 70 % of the keys at one key per bucket) reads one memory line instead of
 * two. A table is in one of two states: LOG (index and log are the truth) or INLINE (the lines are the truth
 * for the inline keys; their log entries are stale until the table returns to LOG). The library converts by
 * itself: to the preferred layout before a launch whose kernels know the lines (64-B entries without RMWs:
 * the local direct launch, unique INV / ACK launches, ACK rows launches, VAL launches), to LOG before every
 * other launch, before a populate and before every export above (hkv_device_index / hkv_device_log wait for
 * the table's streams first; the pointers they return are current until the next launch).
 * hkv_table_prefer_layout sets the sticky preference and returns 1 when the table is eligible (64-B
 * entries, a log that has not wrapped, log_cap <= 2^36, room for 128 B per bucket in device memory), 0 when
 * it is not (the table then stays LOG), negative on error. The default preference is LOG. Once allocated, the
 * lines stay until hkv_table_destroy, also after a preference of LOG. A pointer from hkv_device_index /
 * hkv_device_log that is held across launches goes stale on an INLINE table (the inline keys' log entries
 * are not updated there): call again after the launches, which converts and returns the current image. */
#define HKV_LAYOUT_LOG 0
#define HKV_LAYOUT_INLINE 1
typedef struct hkv_layout_info {
    int32_t state;               /* HKV_LAYOUT_* the table is in now */
    int32_t preferred;           /* HKV_LAYOUT_* */
    int32_t eligible;            /* what hkv_table_prefer_layout(t, HKV_LAYOUT_INLINE) would return now */
    int32_t reserved;
    uint64_t conversions;        /* conversions so far, either way */
    uint64_t inline_launches;    /* launches (batch launches and the workload's table readers) run while INLINE */
    uint64_t line_bytes;         /* device memory of the inline residency (0: not allocated) */
} hkv_layout_info;
int  hkv_table_prefer_layout(hkv_table *t, int layout);
int  hkv_table_layout(hkv_table *t, hkv_layout_info *out);
/* converts to the preferred layout now (as the next inline-capable launch would), on `stream` */
int  hkv_table_apply_layout(hkv_table *t, void *stream);
/* debug export of the inline residency (128 B per bucket, private format: bit 63 of a slot word is the inline
 * flag), in the manner of hkv_copy_index; does not convert. An error while the residency is not allocated. */
int  hkv_copy_lines(hkv_table *t, void *host_dst, uint64_t offset, uint64_t bytes);

/* Table census and digest. One streaming pass over the buckets that reports the table's protocol state: how
 * many keys it holds, in which states, who wrote the ones that are not VALID, the highest timestamp, and a
 * digest of every key's replicated bytes. It reads the table as it is, from whichever residency it is in (a LOG
 * table from index and log, an INLINE table from the lines and, for the keys that are not inline, the log): it
 * converts nothing, and the layout counters (conversions, inline_launches) do not move.
 *
 * A slot is live when it is in use and log_head - offset < log_cap (the lookup's window check); its entry is a
 * live key. Every field is a sum, an xor or a maximum over the live keys, so the result does not depend on the
 * order of buckets, blocks or atomics: equal tables give equal bytes.
 *
 * The digest, keyed by key (not by log position or bucket), with all arithmetic modulo 2^64:
 *   mix64(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *             (the splitmix64 finaliser)
 *   G = 0x9E3779B97F4A7C15
 *   An entry of E bytes (64, or 320 with big objects) is E/8 little-endian 64-bit words w[i]. Keep bytes 8..15
 *   (key), 18 (state), 23 (ts cid), 24..27 (ts version) and 33..33+ST_VALUE_SIZE-1 (value, which ends with the
 *   entry), zero every other byte: the masked words m[i]. m[0] is always zero and is skipped.
 *   e = sum over i >= 1 of mix64(m[i] + (i + 1) * G)
 *   h = mix64(e)
 *   digest_sum = sum over the live keys of h;  digest_xor = xor over the live keys of mix64(h + G)
 * Left out on purpose, being each replica's own: key_first, opcode, val_len, ack_bv, rmw_lwid,
 * op_buffer_index, the lock byte (some engines keep launch tags there between launches, which is also why no
 * "locked" count is offered) and the last-local-write timestamp. Two replicas that hold every key with the same
 * state, timestamp and value have the same digest however their logs were filled. */
typedef struct hkv_census {
    uint64_t keys;               /* live slots: in-use, and log_head - offset < log_cap (the lookup's window check) */
    uint64_t dead_slots;         /* in-use slots whose entry the log has overwritten */
    uint64_t by_state[8];        /* live keys by state byte 1..5 (hermes_states_t); any other value counts in [0] */
    uint64_t obi_set;            /* live keys with op_buffer_index != 255 */
    uint64_t not_valid_by_cid[9];/* live keys not VALID, by ts cid 0..7; [8] = any other cid */
    uint64_t max_ts;             /* max over live keys of (version << 8 | cid) */
    uint64_t digest_sum, digest_xor;
    uint64_t from_lines;         /* live keys whose entry was read from the inline residency (0 while LOG) */
    uint64_t offenders;          /* live keys not VALID (= what the list below would hold with room for all) */
} hkv_census;
uint32_t hkv_census_bytes(void);   /* sizeof(hkv_census), for bindings */

/* asynchronous on stream; d_out: device memory, sizeof(hkv_census), 8-byte aligned, overwritten (not
 * accumulated). d_offender_keys (may be NULL): receives the 8-byte keys of up to offender_cap live keys that are
 * not VALID, in no particular order; entries past min(offenders, offender_cap) are not written. Ordered after
 * the launches already enqueued on the table's last stream; like a launch, one caller at a time per table. A
 * serving kernel of the host-pointer path that is live on the table is stopped first, as by the other hkv_*
 * calls. */
int hkv_table_census_async(hkv_table *t, hkv_census *d_out, uint64_t *d_offender_keys,
                           uint64_t offender_cap, void *stream);
/* the same, synchronous, into host memory, no offender list */
int hkv_table_census(hkv_table *t, hkv_census *host_out);

/* Replica repair (ABI 10): a table's replicated state as records, and their timestamp-guarded install into
 * another table, of either residency and of any geometry (bucket count, log capacity, log order). Where
 * hkv_copy_index / hkv_copy_log ship a byte image -- identical geometry, LOG only, overwriting whatever the
 * target has learnt since -- a record is keyed by key and applied by the protocol's own rules.
 *
 * Record. An entry image of E bytes (64, or 320 with big objects) that keeps exactly the bytes the digest keeps
 * -- key 8..15, state 18, ts cid 23, ts version 24..27, value 33..33+ST_VALUE_SIZE-1 -- and is zero in every
 * other byte. The digest's h of a record is therefore that of the entry it came from, and the sum of h over an
 * unfiltered extract of a whole table is its census's digest_sum.
 *
 * Extract. One record per live slot (the census's definition: in use, and log_head - offset < log_cap) of the
 * buckets [bkt_lo, bkt_hi) whose packed timestamp (version << 8 | cid) is at least min_ts, written compacted to
 * d_records in no particular order. hkv_extract_result.records is the number that qualify and may exceed
 * record_cap: records past record_cap are not written and nothing at or past min(records, record_cap) * E
 * bytes of d_records is touched. d_result is overwritten, not accumulated. The residency rule is the
 * census's: the table is read as it is (an INLINE table's inline keys from their lines, never from their stale
 * log copies), nothing is converted, and the layout counters (conversions, inline_launches) do not move. The
 * bucket range lets a caller stream a large table through a bounded buffer; one extract holds no key twice.
 * min_ts only reduces the volume. Whether leaving out the older keys is sound is the caller's business: the
 * protocol orders writes per key, so there is no global watermark below which a target is known to be current.
 *
 * Install. The result is defined by the reference: installing the n records R into a table equals the
 * reference applying two batches, one after the other, under the table's membership (no field of which these
 * two batch types read):
 *   an `invs` batch of one INV per record -- opcode ST_OP_INV, the record's key, timestamp and value, sender =
 *   the record's ts cid, val_len ST_VALUE_SIZE (as the worker's INVs carry it), RMW flag 0;
 *   then a `vals` batch of one VAL (key, timestamp) for every record whose state byte is VALID.
 * So a record newer than the key's timestamp installs value and timestamp and moves the state as
 * hermes_exec_inv does (VALID at the end when the source was VALID); a record of equal timestamp touches only
 * what an INV and a VAL of that timestamp touch; an older record changes nothing; a key the source caught
 * mid-write (state not VALID) is left not VALID at that timestamp -- the message a shadow replica would have
 * received; a key the target does not hold is a miss (there are no inserts after populate; hkv_table_upsert, below, is the
 * install that inserts such a key). The lock byte,
 * ack_bv, op buffer index and last-local-write timestamp are left as those two batches leave them, and the
 * per-line F/X/Y/T words of the batch engines are not touched. On an INLINE table the inline keys are read and
 * written in their lines only; nothing is converted and the layout counters do not move.
 * The caller guarantees that no key occurs twice among the n records (as for HKV_BATCH_UNIQUE: each record is
 * then its key's only one and is applied in a single pass, in any order); the records of one extract have this
 * property. A duplicate breaks the result.
 * hkv_install_result counts, against the table as it was before the call: raised (record ts > key ts), equal,
 * older and missed; d_result is overwritten.
 *
 * Both calls are asynchronous on `stream`, ordered after the launches already enqueued on the table's last
 * stream, one caller at a time per table, and stop a live serving kernel of the host-pointer path first (as
 * hkv_table_census_async). Both refuse, with a negative code and a message in hkv_last_error() before
 * anything is launched: a table with rmw_enabled (a record carries no RMW flag, and an RMW build's INVs
 * depend on it); d_records or d_result not 16-byte aligned; bkt_hi > num_bkts or bkt_lo > bkt_hi.
 * Out of scope: re-admitting the repaired replica to the membership. A repair is sound while the target takes
 * no client operations; INVs it receives meanwhile are safe, the install being timestamp-guarded. */
typedef struct hkv_extract_result {
    uint64_t records;            /* records that qualify (may exceed record_cap) */
    uint64_t scanned_keys;       /* live slots of the bucket range, whatever their timestamp */
} hkv_extract_result;
typedef struct hkv_install_result {
    uint64_t raised;             /* record ts > key ts: value, timestamp and state installed */
    uint64_t equal;              /* record ts == key ts */
    uint64_t older;              /* record ts < key ts: nothing changed */
    uint64_t missed;             /* the table does not hold the key */
} hkv_install_result;
uint32_t hkv_extract_result_bytes(void);   /* sizeof, for bindings */
uint32_t hkv_install_result_bytes(void);
int hkv_table_extract_async(hkv_table *t, uint64_t bkt_lo, uint64_t bkt_hi, uint64_t min_ts, void *d_records,
                            uint64_t record_cap, hkv_extract_result *d_result, void *stream);
int hkv_table_install_async(hkv_table *t, const void *d_records, uint64_t n, hkv_install_result *d_result,
                            void *stream);

/* Partitioned census and delta repair (ABI 10, functions only): anti-entropy by key range. The census says that
 * two replicas differ, not where, so a repair ships every key. Here both sides take the census per partition of
 * the key space, the rows are compared, and only the partitions that differ are extracted and installed.
 *
 * Partition. For part_bits b and P = 2^b, key k lies in partition k & (P - 1). A key's bucket is
 * k & 0xFFFFFFFFFFFF & (num_bkts - 1), so with P <= num_bkts -- the rule part_bits <= log2(num_bkts), which
 * every call below enforces -- a bucket's number has the same low b bits as every key in it: all keys of a bucket
 * lie in one partition, on any table with at least P buckets, whatever its bucket count, log order or residency.
 * Two replicas compare rows taken with the same part_bits; their geometries need not agree.
 *
 * hkv_table_census_parts_async. rows[p], p < P, holds the census's digest_sum, digest_xor, keys and offenders
 * (here: not_valid) restricted to the live keys of partition p; d_rows is P rows of device memory, 16-byte
 * aligned, overwritten, not accumulated. Over p the rows fold to the census: digest_sum by addition modulo 2^64,
 * digest_xor by xor, keys and not_valid by addition (to keys and offenders); part_bits 0 gives one row equal to
 * those four census fields. Liveness, residency and ordering are the census's: a slot is live when it is in use
 * and log_head - offset < log_cap; the table is read as it is (an INLINE table's inline keys from their lines,
 * never from their stale log copies); nothing is converted and conversions / inline_launches do not move; the
 * call is asynchronous on `stream`, ordered after the table's last stream, takes one caller at a time, and stops
 * a live serving kernel first. Every field is a sum or an xor, so equal tables give equal bytes, and a second
 * call into the same buffer gives the same bytes. Tables with RMWs are accepted, as by the census.
 *
 * hkv_part_rows_diff_async. d_mask[p] = 1 where rows a and b differ in any of the four words, else 0; with
 * accumulate != 0 the byte that is there is or-ed with that instead (the union over several peers). *d_count =
 * the non-zero bytes of d_mask afterwards. No table is involved: it is ordered by `stream` alone.
 *
 * hkv_table_extract_parts_async. hkv_table_extract_async restricted to the buckets of [bkt_lo, bkt_hi) whose
 * partition b & (P - 1) has a non-zero byte in d_part_mask (P bytes; any non-zero value selects). An unselected
 * bucket is not read: scanned_keys counts the live slots of the selected buckets of the range only. records,
 * record_cap and "nothing at or past min(records, record_cap) * E is touched" are the extract's. With min_ts 0
 * and the whole bucket range, records is the sum of rows[p].keys over the selected partitions.
 *
 * Refusals, with a negative code and a message in hkv_last_error() that names the call, before anything is
 * launched: a NULL table (or rows, mask, count); part_bits > log2(num_bkts); rows not 16-byte aligned; for the
 * masked extract everything hkv_table_extract_async refuses (RMW tables among it) and a NULL mask.
 *
 * A delta repair (hermes_amd.replica_group.delta_resync) is: both partition censuses, the diff, the masked
 * extract of the source, the install into the target, and the target's partition census again. Shipping a whole
 * differing partition is harmless for its keys that were equal, the install being timestamp-guarded. Every limit
 * of a repair holds: the target takes no client operations meanwhile, nothing is inserted, nobody is re-admitted
 * to the membership, and extract and install refuse RMW tables. A partition can still differ afterwards, and is
 * then reported, not hidden; two causes are known: the target is newer in a key (that record counts as `older`),
 * or the target lacks the key or shadows it behind another (that record counts as `missed`; a delta repair that
 * upserts instead of installing, hkv_table_upsert below, inserts it). */
typedef struct hkv_part_row {
    uint64_t digest_sum, digest_xor;   /* the census's, over the partition's live keys */
    uint64_t keys;                     /* live keys of the partition */
    uint64_t not_valid;                /* of them, not VALID (adds up to hkv_census.offenders) */
} hkv_part_row;
uint32_t hkv_part_row_bytes(void);   /* sizeof(hkv_part_row) = 32, for bindings */
int hkv_table_census_parts_async(hkv_table *t, uint32_t part_bits, hkv_part_row *d_rows, void *stream);
int hkv_part_rows_diff_async(const hkv_part_row *d_a, const hkv_part_row *d_b, uint32_t part_bits,
                             uint8_t *d_mask, uint64_t *d_count, int accumulate, void *stream);
int hkv_table_extract_parts_async(hkv_table *t, uint32_t part_bits, const uint8_t *d_part_mask,
                                  uint64_t bkt_lo, uint64_t bkt_hi, uint64_t min_ts, void *d_records,
                                  uint64_t record_cap, hkv_extract_result *d_result, void *stream);

/* Upsert (ABI 10, functions only): install records and insert the keys the table lacks. The install and the delta
 * repair above stop at a key the target does not hold; hkv_table_upsert takes the same records (device memory,
 * 16-byte aligned, n records of E bytes, no key twice -- the caller's guarantee -- and never written by the call)
 * and inserts those keys as the reference inserts: mica_insert_one. The result goes to HOST memory and the call
 * returns when its work on `stream` is done, as hkv_table_populate does: the table's log head lives on the host and
 * the number of inserts is known only on the device.
 *
 * An upsert equals the reference doing the following.
 *   1. Install. The install of the n records exactly as defined under "Replica repair": one `invs` batch, then one
 *      `vals` batch. A record whose INV comes back ST_MISS is missed; the missed set is decided here, against the
 *      table as it was before the call.
 *   2. Insert. Then, for each missed record in record order: mica_insert_one (mica.c:78-146) of the entry image
 *      that spacetime_populate_fixed_len(kv, ., KVS_VALUE_SIZE) builds (spacetime.c:17-68: opcode ST_OP_PUT, val_len
 *      KVS_VALUE_SIZE >> SHIFT_BITS, state VALID, last writer 127, op buffer index 255, timestamp (0, 255); the
 *      fields the reference leaves uninitialised -- ack_bv, RMW flag, last-local-write timestamp -- zero, as a
 *      populate writes them), with two changes: bytes 8..15 are the record's key with bytes 0..7 zero (a record
 *      carries no key_first, and no lookup reads it), and the value bytes are the record's value. Immediately
 *      afterwards the reference applies that record's INV and, if its state byte is VALID, its VAL, as one-element
 *      batches, which find the entry just inserted (*). So the entry that lands in the log is a pure function of the
 *      record, also when a later insert of the same call replaces its slot: a record newer than (0, 255) leaves
 *      its timestamp, last writer = its cid, val_len KVS_VALUE_SIZE as an INV writes it, and state VALID when the
 *      record was VALID, else INVALID (a key the source held mid-write arrives INVALID with the writer's cid as last
 *      writer); a record of timestamp (0, 255) -- a key never written -- leaves the populate image; an older one
 *      (version 0, cid < 255) leaves the populate image too, VALID.
 *      The i-th missed record, counting in record order, takes the i-th log offset mica_insert_one would hand out
 *      from the current head: the head advances by E (the 8-byte rounding of the copied length) per insert and
 *      wraps once, when no more than KVS_VALUE_SIZE + 32 bytes remain below log_cap; after that wrap the unsigned
 *      test never fires again. Slot choice is the reference's: the last slot of the bucket that is empty or carries
 *      the key's tag, else slot tag & 7. Within a bucket the inserts are applied in record order.
 *      (*) The lookup takes the first in-use slot with the key's tag, the insert the last slot that is empty or
 *      has it. On a table filled by inserts alone they are the same slot: the slots fill from slot 7 downwards, so
 *      the empty ones lie below the ones in use, and a tag is never in use twice in a bucket.
 * Index, log and log head after the call are therefore bytes a model can predict (tests/upsert_model.py): they do
 * not depend on grid size, block order or atomics.
 *
 * hkv_upsert_result (64 bytes): raised, equal, older -- the install's counts; inserted -- the install's `missed`;
 * replaced -- inserts that took an in-use slot by tag match: the key that slot pointed to, if it was live and a
 * different key, is no longer reachable (the reference's lossy index; it is what makes ids 631343 / 722989 / 864394
 * miss at 1M keys); evictions -- inserts that found no slot and took slot tag & 7 (also added to what
 * hkv_num_index_evictions reports); log_head -- the log head after the call; one reserved word, zero.
 *
 * Residency. Step 1 runs on the table as it is, LOG or INLINE, exactly like the install. If nothing was missed the
 * call ends there and is indistinguishable from an install: conversions and inline_launches do not move. If
 * anything was missed the table goes to LOG first (as before a populate) and the inserts go into index and log;
 * the next inline-capable launch reconverts by the sticky preference, as after a populate. Inserting into the
 * lines in place is out of scope: every insert into a bucket that is not full takes a slot below the ones in use
 * and so would change the bucket's inline key.
 * The table's insert count and log head advance; a wrapped log makes the table ineligible for the inline layout,
 * as after a populate. The per-line F/X/Y/T words of the batch engines are not touched (DESIGN 4.12 has the
 * argument why a line first used, or reused after a wrap, needs nothing).
 * Ordering: a live serving kernel is stopped and the call is ordered after the table's last stream, as the other
 * table calls; one caller at a time per table.
 * Refusals, with a negative code and a message that names `upsert`, before anything is launched: a NULL table,
 * records (whatever n is) or result; a table with rmw_enabled (the install's reason); records not 16-byte aligned;
 * n above 2^31 - 1. Every entry size is supported: 64 B and E = 64 + 64 c. Out of scope: re-admitting the rebuilt
 * replica to the membership, and a client-facing insert opcode in the batch path (the reference has none). */
typedef struct hkv_upsert_result {
    uint64_t raised, equal, older;   /* the install's counts, against the table as it was before the call */
    uint64_t inserted;               /* the install's missed: every one of them was inserted */
    uint64_t replaced;               /* inserts that took an in-use slot by tag match */
    uint64_t evictions;              /* inserts that found no slot (slot tag & 7) */
    uint64_t log_head;               /* the log head after the call */
    uint64_t reserved;               /* zero */
} hkv_upsert_result;
uint32_t hkv_upsert_result_bytes(void);   /* sizeof(hkv_upsert_result) = 64, for bindings */
int hkv_table_upsert(hkv_table *t, const void *d_records, uint64_t n, hkv_upsert_result *host_result, void *stream);
/* timing hook (tools/rebuild_bench.py): with HKV_UPSERT_PHASES set in the environment every upsert records an event
 * between its phases, and this returns the table's last upsert's times in ms: the install pass, the scan and the
 * pairs, the sort, the bucket replay, the log writes (the last four zero when nothing was inserted). An error
 * without the variable. */
int hkv_debug_upsert_phases(const hkv_table *t, float *ms5);

/* Key-level delta repair (ABI 10, functions only): key summaries first, then only the records needed. The
 * partition rows say where two replicas differ, never which key, so a delta repair ships every record of a differing
 * partition. Three read-only calls close the gap: the source sends a 16-byte summary per key of those partitions,
 * the target answers with the keys it needs, and the source sends the records of those keys alone.
 *
 * Summary (hkv_key_summary, 16 bytes): bytes 0..7 the key (entry bytes 8..15), 8..11 the ts version, 12 the ts cid,
 * 13 the state byte, 14..15 zero. A summary is a function of its record (and so of the entry's digest bytes).
 *
 * hkv_table_summaries_async. One summary per live slot that hkv_table_extract_parts_async with the same part_bits,
 * mask, bucket range and min_ts would emit a record for, compacted to d_summaries in no particular order. A NULL
 * d_part_mask selects every partition (part_bits is still checked). records, scanned_keys, cap and "nothing at or
 * past min(records, cap) * 16 bytes is touched" mean what they mean for the extract. Only the first 32 bytes of
 * an entry are read, whatever the entry size.
 *
 * hkv_table_need_async. Each of the n summaries is looked up as the reference looks a key up (first in-use tag
 * match, window check, 8-byte key compare) and classed against the table's entry, by packed timestamp
 * (version << 8 | cid):
 *   missed      the table does not hold the key
 *   newer       summary ts > entry ts
 *   validate    equal ts, summary state VALID, entry state not VALID
 *   same        equal ts and equal state byte
 *   state_only  equal ts, the state bytes differ, and an install would not change the entry's state (the summary's
 *               state is not VALID)
 *   older       summary ts < entry ts
 * THE RULE: a key is *needed* exactly when installing its record would miss, or would change a byte of the entry
 * that the digest keeps. That is missed, newer and validate: a newer record installs timestamp, value and state; a
 * record of equal timestamp changes a digest byte only through its VAL, which sets the state to VALID where it was
 * not; an older record changes nothing. (An equal record also rewrites the last-writer bits, which the digest leaves
 * out.) The needed keys, 8 bytes each, are written compacted to d_need_keys in no particular order; `needed` may
 * exceed need_cap, and nothing at or past min(needed, need_cap) * 8 bytes is touched. d_result is overwritten, not
 * accumulated. Nothing is written to the table, so a key may occur any number of times among the summaries (each
 * occurrence is classed and, if needed, listed).
 *
 * hkv_table_fetch_async. Positional: record i, at d_records + i * E, is the record (see "Replica repair": the entry
 * image under the digest's mask) of key d_keys[i]. A key the table does not hold gives a record that is zero but for
 * the key in bytes 8..15 (state 0 is no hermes state: such a record is recognisable). A key may occur any number of
 * times. found + absent = n.
 *
 * All three follow the census's rules: the table is read as it is (an INLINE table's inline keys from their lines,
 * never from their stale log copies); nothing is converted and conversions / inline_launches do not move; the call is
 * asynchronous on `stream`, ordered after the table's last stream, takes one caller at a time, and stops a live
 * serving kernel first. None writes the table. Refusals, with a negative code and a message in hkv_last_error() that
 * names the call (summaries, need, fetch), before anything is launched: a NULL table or result; a NULL buffer whose
 * count (cap, n, need_cap) is not zero; a buffer or result that is not 16-byte aligned; a table with rmw_enabled (the
 * extract's reason: what these calls produce feeds the install); for the summaries also bkt_hi > num_bkts,
 * bkt_lo > bkt_hi and part_bits > log2(num_bkts).
 *
 * A key-level repair (hermes_amd.replica_group.key_delta_resync) is: both partition censuses and the diff, as in
 * a delta repair; the source's summaries of the differing partitions; the target's need list; the source's fetch
 * of it; the install (or the upsert) into the target; the target's partition census again. It ships 16 bytes per
 * key of the differing partitions, 8 per needed key and E per needed key, where the delta repair ships E per key
 * of the differing partitions. Every limit of a repair holds. */
typedef struct hkv_key_summary {
    uint64_t key;                /* entry bytes 8..15 */
    uint32_t ts_version;
    uint8_t  ts_cid;
    uint8_t  state;
    uint8_t  zero[2];
} hkv_key_summary;
typedef struct hkv_need_result {
    uint64_t missed, newer, validate;   /* the needed classes */
    uint64_t same, state_only, older;   /* the others */
    uint64_t needed;                    /* missed + newer + validate (may exceed need_cap) */
    uint64_t reserved;                  /* zero */
} hkv_need_result;
typedef struct hkv_fetch_result {
    uint64_t found;              /* keys the table holds */
    uint64_t absent;             /* keys it does not: zero records but for the key */
} hkv_fetch_result;
uint32_t hkv_key_summary_bytes(void);    /* sizeof(hkv_key_summary) = 16, for bindings */
uint32_t hkv_need_result_bytes(void);    /* sizeof(hkv_need_result) = 64 */
uint32_t hkv_fetch_result_bytes(void);   /* sizeof(hkv_fetch_result) = 16 */
int hkv_table_summaries_async(hkv_table *t, uint32_t part_bits, const uint8_t *d_part_mask, uint64_t bkt_lo,
                              uint64_t bkt_hi, uint64_t min_ts, void *d_summaries, uint64_t cap,
                              hkv_extract_result *d_result, void *stream);
int hkv_table_need_async(hkv_table *t, const void *d_summaries, uint64_t n, uint64_t *d_need_keys, uint64_t need_cap,
                         hkv_need_result *d_result, void *stream);
int hkv_table_fetch_async(hkv_table *t, const uint64_t *d_keys, uint64_t n, void *d_records,
                          hkv_fetch_result *d_result, void *stream);

/* Sketch-level delta repair (ABI 10, functions only): an invertible sketch where the key-level repair ships
 * summaries. The partition rows cannot say which key of a differing partition differs, so a key-level repair ships
 * the summary of every key of such a partition. With an invertible Bloom lookup table both sides fold their
 * summaries of those partitions into a small table of cells, one table is shipped, the two are subtracted, and the
 * difference is peeled: it yields exactly the summaries one side has and the other lacks. The bytes follow the
 * number of differing keys, not the number of keys near them. No table is involved in either call.
 *
 * All arithmetic is modulo 2^64. mix64 and G are the census's (the splitmix64 finaliser, 0x9E3779B97F4A7C15).
 *
 * Element: a hkv_key_summary read as two little-endian words, a = bytes 0..7 (the key), b = bytes 8..15 (ts version,
 * ts cid, state, two zero bytes).
 * Check word: c(a, b) = mix64(mix64(a + G) + b).
 * Sketch: 3 S cells, three subtables of S cells each, 1 <= S < 2^32; S need not be a power of two.
 * Slot: an element's cell in subtable j (0, 1, 2) is j S + (((mix64(c + (j + 1) G) >> 32) * S) >> 32). The slots
 * depend on c, so two versions of one key (another timestamp or state) fall into unrelated cells.
 * Cell (hkv_sketch_cell, 32 bytes): count, key_xor, meta_xor, check_xor. Adding an element does count += 1,
 * key_xor ^= a, meta_xor ^= b, check_xor ^= c in its three cells. The sketch of a list is the sum over its elements:
 * a function of the multiset, whatever the list's order, the grid or the order the atomics land in, so equal lists
 * give equal bytes.
 * Difference: D = A - B cell by cell; the counts are subtracted, the other three words xor-ed.
 * Pure cell: cell i of subtable j is pure when count is 1 or 2^64 - 1, c(key_xor, meta_xor) == check_xor, and the
 * slot of the element (key_xor, meta_xor) in subtable j is i.
 *
 * Decode. Passes p = 0, 1, 2, ...; pass p looks at subtable p mod 3 only. Every cell of that subtable that is pure
 * as the pass begins gives up its element: to the only_a list when count is 1, to only_b when it is 2^64 - 1. The
 * element is then taken out of its three cells (their counts lose the pure cell's count, the other words are
 * xor-ed); the pure cell becomes zero. Within a pass no element is taken twice, an element having one cell per
 * subtable, and the other two subtables are only written, by commutative updates. So the cell bytes after every
 * pass, the pass count and the two lists as sets are fixed by D alone; grid size and scheduling do not change them.
 * The decode ends after three consecutive passes that found nothing, or at HKV_SKETCH_MAX_PASSES (a cap, not a
 * tuning knob: 2.0 n cells decode n elements in about a dozen passes, 1.3 n cells in under fifty).
 *
 * Result (hkv_sketch_result, 64 bytes): only_a, only_b -- the elements taken; either may exceed its cap, elements
 * past a cap are still taken out of the cells, and nothing is written at or past min(count, cap) * 16 bytes of a
 * list. undecoded -- the non-zero cells left; 0: the decode is complete. passes -- the index of the last pass that
 * took an element, plus 1; 0 when none did. exhausted -- 1 when the decode stopped at HKV_SKETCH_MAX_PASSES without
 * three consecutive passes that found nothing (passes > HKV_SKETCH_MAX_PASSES - 3). The reserved words are zero.
 * d_a is left holding the remainder, the 2-core of the difference.
 *
 * Safety. A false pure cell needs a 64-bit check collision. Even then it cannot corrupt a table: decoded summaries
 * only feed hkv_table_need_async and hkv_table_fetch_async, which read the real tables; a bogus key comes back
 * absent, and a bogus version of a real key fetches that key's real record, whose install is timestamp-guarded.
 *
 * hkv_summaries_sketch_async: one pass over n summaries into d_cells (3 * sub_cells cells). accumulate == 0: the
 * cells are zeroed first (overwritten, not accumulated); otherwise the list is added to what is there.
 * hkv_sketch_decode_async: d_a -= d_b, then the passes, all enqueued up front with no host read in between; a pass
 * that follows three idle ones returns at once. d_result is overwritten. Both calls are asynchronous and ordered by
 * `stream` alone. Refusals, with a negative code and a message in hkv_last_error() that names the call (sketch,
 * sketch_decode), before anything is launched: a NULL cells buffer or result; a NULL buffer whose count or cap is
 * not zero; a buffer or result that is not 16-byte aligned; sub_cells == 0 or >= 2^32.
 *
 * A sketch-level repair (hermes_amd.replica_group.sketch_delta_resync) is: both partition censuses and the diff;
 * summaries of the source and of the target for the differing partitions; one sketch of each with the same S; the
 * decode of source minus target at the target; the target's need list of only_a; the source's fetch; the install
 * (or the upsert); the target's partition census again. It ships 96 S bytes of sketch where the key-level repair
 * ships 16 bytes per key of the differing partitions. When undecoded != 0 the lists are dropped and the key-level
 * exchange runs instead. Every limit of a repair holds. */
#define HKV_SKETCH_MAX_PASSES 192
typedef struct hkv_sketch_cell {
    uint64_t count, key_xor, meta_xor, check_xor;
} hkv_sketch_cell;
typedef struct hkv_sketch_result {
    uint64_t only_a, only_b;     /* elements taken (either may exceed its cap) */
    uint64_t undecoded;          /* non-zero cells left */
    uint64_t passes;             /* index of the last pass that took an element, plus 1 */
    uint64_t exhausted;          /* 1: stopped at HKV_SKETCH_MAX_PASSES */
    uint64_t reserved[3];        /* zero */
} hkv_sketch_result;
uint32_t hkv_sketch_cell_bytes(void);     /* sizeof(hkv_sketch_cell) = 32, for bindings */
uint32_t hkv_sketch_result_bytes(void);   /* sizeof(hkv_sketch_result) = 64 */
int hkv_summaries_sketch_async(const void *d_summaries, uint64_t n, hkv_sketch_cell *d_cells, uint64_t sub_cells,
                               int accumulate, void *stream);
int hkv_sketch_decode_async(hkv_sketch_cell *d_a, const hkv_sketch_cell *d_b, uint64_t sub_cells, void *d_only_a,
                            uint64_t cap_a, void *d_only_b, uint64_t cap_b, hkv_sketch_result *d_result, void *stream);

/* default table used by the reference entry points */
int  hkv_set_default_config(const hkv_config *cfg);
hkv_table *hkv_default_table(void);

/* test hooks of the host entry point's combining submit: with a hold of n, the caller that
 * assembles the next launch first waits (up to 5 s) until n batches are queued, so a test can put
 * batches from several threads into one launch in a known order; 0 (default) = no hold. queued =
 * batches waiting in the default table's queue now. */
int  hkv_debug_host_hold(int n_batches);
int  hkv_debug_host_queued(void);

/* synthetic workload helpers (device kernels) */
/* keys_second[i] = CityHash128(&id_i, 4).second for ids[i] (mica_gen_keys, mica.c:149-165) */
int  hkv_hash_ids(const uint32_t *d_ids, uint64_t *d_keys_second, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HERMESKV_H */
