"""Host-side mirror of the reference's KVS interface, on top of libhermeskv.so.

Two ways in, matching the two halves of include/hermeskv.h:

* reference entry points -- `spacetime_init`, `spacetime_populate_fixed_len`,
  `hermes_batch_ops_to_KVS` -- same names, argument meaning and error behaviour as
  include/hermes/spacetime.h:211-230 (they call the exported C symbols: the drop-in path);
* `HermesKV`, one HBM-resident table per replica with the device fast path: many batches
  (one per virtual worker) concatenated into one launch on torch tensors, on torch's stream.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import layout as L
from .lib import (ABI_VERSION, HkvBatchDesc, HkvCensus, HkvConfig, HkvError, HkvLayoutInfo, HkvUpsertResult, Membership,
                  check, raw)

_L = raw()


def _membership_struct(mb: bytes) -> Membership:
    return Membership(int.from_bytes(bytes(mb[:8]).ljust(8, b"\0"), "little"))


# ---------------------------------------------------------------- reference entry points
def set_default_config(**kw) -> None:
    """hkv_set_default_config: must precede spacetime_init (e.g. machine_id, num_keys, rmw)."""
    cfg = make_config(**kw)
    check(_L.hkv_set_default_config(ctypes.byref(cfg)), "hkv_set_default_config")


def spacetime_init(instance_id: int) -> None:
    """spacetime.h:211 -- build and populate the default table in HBM."""
    _L.spacetime_init(int(instance_id))


def spacetime_populate_fixed_len(n: int, val_len: int) -> None:
    """spacetime.h:212."""
    _L.spacetime_populate_fixed_len(None, int(n), int(val_len))


def hermes_batch_ops_to_KVS(btype: int, op_array: np.ndarray, op_num: int, sizeof_op_elem: int,
                            curr_membership: bytes, node_suspected: list | None,
                            read_write_ops: np.ndarray | None, thread_id: int = 0) -> None:
    """spacetime.h:228-230 on host numpy arrays, mutated in place. `node_suspected` is a
    one-element list standing for the int* out-parameter (or None for NULL). As in the
    reference, read_write_ops must hold the table's rw_len (max_batch_size, 250) ops."""
    assert op_array.flags["C_CONTIGUOUS"]
    ns = ctypes.c_int(node_suspected[0] if node_suspected else -1)
    _L.hermes_batch_ops_to_KVS(int(btype), op_array.ctypes.data_as(ctypes.c_void_p), int(op_num),
                               int(sizeof_op_elem), _membership_struct(curr_membership),
                               ctypes.byref(ns) if node_suspected is not None else None,
                               read_write_ops.ctypes.data_as(ctypes.c_void_p) if read_write_ops is not None else None,
                               int(thread_id))
    if node_suspected is not None:
        node_suspected[0] = ns.value


# ---------------------------------------------------------------- tables
def make_config(num_keys: int = 1_000_000, num_bkts: int = 2 * 1024 * 1024, log_cap: int = 1 << 30,
                machine_id: int = 0, rmw: bool = False, big_objects: bool = False,
                extra_cache_lines: int = 0, device: int = 0, rw_len: int = 250, skew: int = 0) -> HkvConfig:
    """skew: hkv_config.skew_flags (SKEW_READ_COMPLETE | SKEW_WRITE_COALESCE, config.h:79-80)"""
    return HkvConfig(ABI_VERSION, machine_id, int(rmw), int(big_objects), int(extra_cache_lines), device, rw_len,
                     int(skew), num_keys, num_bkts, log_cap)


SKEW_READ_COMPLETE = 1    # ENABLE_READ_COMPLETE_AFTER_VAL_RECV_OF_HOT_REQS (include/hermeskv.h)
SKEW_WRITE_COALESCE = 2   # ENABLE_WRITE_COALESCE_TO_THE_SAME_KEY_IN_SAME_NODE


def sized_geometry(num_keys: int, sizes: L.Sizes = L.DEFAULT) -> tuple[int, int]:
    """Buckets and log capacity for `num_keys` (powers of two; about 2 keys per bucket as in
    the reference's 1M keys / 2^21 buckets, at most 2^27 buckets up to 2^28 keys and 2^29
    beyond (1B keys per replica: 32 GiB of index), and a log that never wraps)."""
    bkts = 1 << max(4, (2 * num_keys - 1).bit_length())
    need = num_keys * sizes.entry + sizes.kvs_value + 64
    cap = 1 << max(16, (need - 1).bit_length())
    return min(bkts, 1 << (27 if num_keys <= 1 << 28 else 29)), cap


LAYOUT_LOG = 0      # hkv_table_prefer_layout (include/hermeskv.h, "Table layouts")
LAYOUT_INLINE = 1   # a private 128-B line per bucket: the bucket and its first key's entry

BATCH_ENGINE = 1   # hkv_batch_desc.flags (include/hermeskv.h): the multi-kernel engine
BATCH_SMALL = 2    # the single-workgroup kernel (launches of at most 4096 elements)
BATCH_PACKED = 4   # INV / VAL batches back to back, d_counts = n_batches + 1 offsets
BATCH_UNIQUE = 8   # no key twice in the launch (INV batches: one pass)
BATCH_ROWS = 16    # with BATCH_UNIQUE: rows of one layout, element j of every row on one key


CENSUS_WORDS = ctypes.sizeof(HkvCensus) // 8
# hkv_census's fields as (first word, words) of its 64-bit words
CENSUS_FIELDS = {name: (getattr(HkvCensus, name).offset // 8, getattr(HkvCensus, name).size // 8)
                 for name, _ in HkvCensus._fields_}


def _census_dict(raw: bytes) -> dict:
    w = np.frombuffer(raw, dtype="<u8")
    return {name: int(w[a]) if n == 1 else [int(x) for x in w[a:a + n]] for name, (a, n) in CENSUS_FIELDS.items()}


@dataclasses.dataclass
class Census:
    """The result of HermesKV.census(), still on the device. `tensor`: hkv_census's CENSUS_WORDS 64-bit words as
    int64 (the unsigned words' bit patterns), `offender_keys`: the key list, or None. Nothing is read back until
    asked: field(name) is a device view for code that stays on the stream (a collective, a comparison), host()
    and the attributes named like hkv_census's fields (keys, by_state, digest_sum, ...) synchronise and return
    Python integers."""
    tensor: torch.Tensor
    offender_keys: torch.Tensor | None = None

    def field(self, name: str) -> torch.Tensor:
        a, n = CENSUS_FIELDS[name]
        return self.tensor[a:a + n]

    def host(self) -> dict:
        return _census_dict(self.tensor.cpu().numpy().tobytes())

    def __getattr__(self, name: str):
        if name in CENSUS_FIELDS:
            return self.host()[name]
        raise AttributeError(name)

    def offenders_host(self) -> np.ndarray:
        """the listed keys (uint64), min(offenders, the list's capacity) of them, in no particular order"""
        if self.offender_keys is None:
            return np.empty(0, np.uint64)
        n = min(self.host()["offenders"], self.offender_keys.numel())
        return self.offender_keys[:n].cpu().numpy().view(np.uint64)


@dataclasses.dataclass
class Extract:
    """The result of HermesKV.extract(), still on the device. `tensor`: the record buffer (uint8, cap x E: each
    record an entry image under the digest's mask, include/hermeskv.h "Replica repair"), `result`:
    hkv_extract_result as two int64 words. Nothing is read back until a count is asked for: records (how many
    qualified, possibly more than the buffer holds), scanned_keys and written = min(records, cap) synchronise."""
    tensor: torch.Tensor
    result: torch.Tensor
    entry: int

    @property
    def cap(self) -> int:
        return self.tensor.numel() // self.entry

    def host(self) -> dict:
        r, s = (int(x) & 0xFFFFFFFFFFFFFFFF for x in self.result.cpu().tolist())
        return {"records": r, "scanned_keys": s}

    @property
    def records(self) -> int:
        return self.host()["records"]

    @property
    def scanned_keys(self) -> int:
        return self.host()["scanned_keys"]

    @property
    def written(self) -> int:
        return min(self.records, self.cap)

    def records_host(self) -> np.ndarray:
        """the written records as [written][E] uint8, in no particular order"""
        n = self.written
        return self.tensor[:n * self.entry].cpu().numpy().reshape(n, self.entry)


SUMMARY_BYTES = 16   # hkv_key_summary
SUMMARY_DTYPE = np.dtype([("key", "<u8"), ("ts_ver", "<u4"), ("ts_cid", "u1"), ("state", "u1"), ("zero", "u1", (2,))])
NEED_FIELDS = ("missed", "newer", "validate", "same", "state_only", "older", "needed")   # hkv_need_result's words
FETCH_FIELDS = ("found", "absent")


@dataclasses.dataclass
class Summaries(Extract):
    """The result of HermesKV.summaries(), still on the device: an Extract whose buffer holds 16-byte key summaries
    (include/hermeskv.h "Key-level delta repair": key, ts version, ts cid, state) instead of records; `entry` is
    16. records, scanned_keys and written mean what they mean there and synchronise."""

    def summaries_host(self) -> np.ndarray:
        """the written summaries as a SUMMARY_DTYPE array, in no particular order"""
        return self.records_host().reshape(-1).view(SUMMARY_DTYPE)


@dataclasses.dataclass
class Need:
    """The result of HermesKV.need(), still on the device. `keys`: int64[cap], of which the first min(needed, cap)
    are the needed keys in no particular order; `result`: hkv_need_result's first seven words as int64 (missed,
    newer, validate, same, state_only, older, needed). host() and the attributes of those names synchronise."""
    keys: torch.Tensor
    result: torch.Tensor

    def host(self) -> dict:
        return {k: int(x) & 0xFFFFFFFFFFFFFFFF for k, x in zip(NEED_FIELDS, self.result.cpu().tolist())}

    def __getattr__(self, name: str):
        if name in NEED_FIELDS:
            return self.host()[name]
        raise AttributeError(name)

    @property
    def written(self) -> int:
        return min(self.host()["needed"], self.keys.numel())

    def keys_host(self) -> np.ndarray:
        """the listed keys (uint64), min(needed, capacity) of them, in no particular order"""
        return self.keys[:self.written].cpu().numpy().view(np.uint64)


@dataclasses.dataclass
class Fetch:
    """The result of HermesKV.fetch(), still on the device. `tensor`: uint8[n x E], record i the record of key i
    (zero but for its key bytes where the table does not hold the key); `result`: found, absent as int64.
    host() and the two attributes synchronise."""
    tensor: torch.Tensor
    result: torch.Tensor
    entry: int

    def host(self) -> dict:
        return {k: int(x) & 0xFFFFFFFFFFFFFFFF for k, x in zip(FETCH_FIELDS, self.result.cpu().tolist())}

    def __getattr__(self, name: str):
        if name in FETCH_FIELDS:
            return self.host()[name]
        raise AttributeError(name)

    def records_host(self) -> np.ndarray:
        """the records as [n][E] uint8, in key order"""
        return self.tensor.cpu().numpy().reshape(-1, self.entry)


PART_FIELDS = ("digest_sum", "digest_xor", "keys", "not_valid")   # hkv_part_row's words


@dataclasses.dataclass
class PartRows:
    """The result of HermesKV.census_parts(), still on the device. `tensor`: [P, 4] int64, row p = hkv_part_row of
    partition p (digest_sum, digest_xor, keys, not_valid: the unsigned words' bit patterns), P = 2^part_bits.
    Nothing is read back until asked: field(name) is a device column for code that stays on the stream (a diff, a
    collective, keys[mask].sum()); host() synchronises and returns the rows as uint64 [P, 4]."""
    tensor: torch.Tensor
    part_bits: int

    def field(self, name: str) -> torch.Tensor:
        return self.tensor[:, PART_FIELDS.index(name)]

    def host(self) -> np.ndarray:
        return self.tensor.cpu().numpy().view(np.uint64)


INSTALL_FIELDS = ("raised", "equal", "older", "missed")


@dataclasses.dataclass
class InstallResult:
    """The result of HermesKV.install(), still on the device: hkv_install_result as four int64 words (raised,
    equal, older, missed, counted against the table as it was before the install). host() and the attributes
    of those names synchronise; `tensor` adds up across installs without a host read."""
    tensor: torch.Tensor

    def host(self) -> dict:
        return {k: int(x) & 0xFFFFFFFFFFFFFFFF for k, x in zip(INSTALL_FIELDS, self.tensor.cpu().tolist())}

    def __getattr__(self, name: str):
        if name in INSTALL_FIELDS:
            return self.host()[name]
        raise AttributeError(name)


class HermesKV:
    """One HermesKV replica: a MICA-herd table in HBM plus the batch path on it."""

    default_flags = 0   # hkv_batch_desc.flags for every launch (tests pin one engine or the other)

    def __init__(self, num_keys: int | None = 1_000_000, num_bkts: int | None = None,
                 log_cap: int | None = None, machine_id: int = 0, rmw: bool = False,
                 big_objects: bool = False, extra_cache_lines: int = 0, device: int = 0,
                 rw_len: int = 250, populate: bool = True, skew: int = 0):
        self.sizes = L.Sizes(big_objects, extra_cache_lines if big_objects else 0)
        nk = num_keys or 0
        if num_bkts is None or log_cap is None:
            b, c = sized_geometry(max(nk, 1), self.sizes)
            num_bkts = num_bkts or b
            log_cap = log_cap or c
        self.cfg = make_config(nk, num_bkts, log_cap, machine_id, rmw, big_objects,
                               extra_cache_lines, device, rw_len, skew)
        self.skew = int(skew)
        self.device = device
        self.machine_id = machine_id
        self.rmw = rmw
        self.num_keys = nk
        h = ctypes.c_void_p()
        check(_L.hkv_table_create(ctypes.byref(self.cfg), ctypes.byref(h)), "hkv_table_create")
        self.h = h
        self._owned = True
        # batch launches and populates through this object so far: what a caller read from the table before the
        # count moved (Round's next-round peer timestamps) may be stale
        self.launches = 0
        if populate and nk:
            self.populate(nk, self.sizes.kvs_value)

    @classmethod
    def default_table(cls) -> "HermesKV":
        """Non-owning view of the table the reference entry points use (spacetime_init)."""
        h = _L.hkv_default_table()
        if not h:
            raise RuntimeError("spacetime_init has not been called")
        self = cls.__new__(cls)
        self.h = ctypes.c_void_p(h)
        self._owned = False
        self.launches = 0
        self.cfg = HkvConfig()
        check(_L.hkv_table_config(self.h, ctypes.byref(self.cfg)), "hkv_table_config")
        self.sizes = L.Sizes(bool(self.cfg.big_objects), self.cfg.extra_cache_lines if self.cfg.big_objects else 0)
        self.device, self.machine_id = self.cfg.device, self.cfg.machine_id
        self.rmw, self.num_keys = bool(self.cfg.rmw_enabled), self.cfg.num_keys
        self.skew = self.cfg.skew_flags
        return self

    def close(self) -> None:
        if getattr(self, "h", None) and getattr(self, "_owned", False):
            _L.hkv_table_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup
    def set_skew(self, skew: int) -> None:
        """hkv_table_set_skew: the table's skew optimisations from the next launch on"""
        check(_L.hkv_table_set_skew(self.h, int(skew)), "hkv_table_set_skew")
        self.cfg.skew_flags = int(skew)
        self.skew = int(skew)

    def populate(self, n: int, val_len: int) -> None:
        self.launches += 1
        check(_L.hkv_table_populate(self.h, int(n), int(val_len)), "hkv_table_populate")

    @property
    def log_head(self) -> int:
        return _L.hkv_log_head(self.h)

    @property
    def evictions(self) -> int:
        return _L.hkv_num_index_evictions(self.h)

    # -- device fast path
    def batch(self, btype: int, elems: torch.Tensor, n_batches: int, stride: int, elem_size: int,
              membership: bytes, counts: torch.Tensor | None = None, rw: torch.Tensor | None = None,
              rw_stride_bytes: int = 0, node_suspected: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None, offsets: torch.Tensor | None = None,
              state_out: torch.Tensor | None = None, opcode_in: torch.Tensor | None = None,
              patch: torch.Tensor | None = None, rw_state: torch.Tensor | None = None,
              unique: bool = False, rows: tuple[int, int, int] | None = None,
              ack_out: torch.Tensor | None = None, ack_out_size: int = 16,
              rw_opcodes: torch.Tensor | None = None) -> None:
        """Apply n_batches batches of one type, concatenated in `elems` (uint8, on the GPU),
        in concatenation order, asynchronously on `stream` (default: torch's current).
        offsets (INV / ACK / VAL batches): the batches stored back to back, batch b at elements
        [offsets[b], offsets[b+1]); `stride` is then the total (HKV_BATCH_PACKED). patch (local
        batches): 16 B per element of pending header writes (hkv_batch_desc.d_patch); rw_state (ACK
        batches): the read_write_ops' state-byte mirror, kept up to date by the completions. unique
        (INV batches): no key appears twice in the launch (HKV_BATCH_UNIQUE, one pass). rows (unique INV /
        ACK launches): (n_rows, row_stride, skip_row) -- n_rows launches of this layout, row r at element
        r * row_stride of elems, applied in row order in one pass (HKV_BATCH_ROWS; skip_row -1: none).
        ack_out (unique INV launches): every element's ACK as the worker's ACK callbacks make it,
        ack_out_size bytes each (hkv_batch_desc.d_ack_out); ACK rows launches: the VAL callbacks' output
        in the ACKs' positions. rw_opcodes (ACK batches): the
        read_write_ops' opcode mirror, one byte per slot (hkv_batch_desc.d_opcode_in): completions read the
        opcode there instead of the op."""
        assert elems.is_cuda and elems.dtype == torch.uint8
        total = stride if offsets is not None else n_batches * stride
        if rows is not None:
            assert unique and rows[0] >= 1 and (rows[0] == 1 or rows[1] >= total)
            assert elems.numel() >= ((rows[0] - 1) * rows[1] + total) * elem_size
        else:
            assert elems.numel() >= total * elem_size
        d = HkvBatchDesc()
        d.type = int(btype)
        d.n_batches = int(n_batches)
        d.stride = int(stride)
        d.elem_size = int(elem_size)
        d.flags = self.default_flags | (BATCH_UNIQUE if unique else 0)
        if rows is not None:
            d.flags |= BATCH_ROWS
            d.n_rows, d.row_stride, d.skip_row = int(rows[0]), int(rows[1]), int(rows[2])
        d.d_elems = elems.data_ptr()
        if state_out is not None:   # local batches: the mirror of each element's final state byte
            assert state_out.is_cuda and state_out.dtype == torch.uint8 and state_out.numel() >= n_batches * stride
            d.d_state_out = state_out.data_ptr()
        if opcode_in is not None:   # local batches: the caller's mirror of each element's opcode byte
            assert opcode_in.is_cuda and opcode_in.dtype == torch.uint8 and opcode_in.numel() >= n_batches * stride
            d.d_opcode_in = opcode_in.data_ptr()
        if rw_opcodes is not None:   # ACK batches: the read_write_ops' opcode mirror
            assert opcode_in is None and rw is not None and rw_opcodes.is_cuda and rw_opcodes.dtype == torch.uint8
            assert rw_opcodes.numel() >= n_batches * (rw_stride_bytes // self.sizes.op)
            d.d_opcode_in = rw_opcodes.data_ptr()
        if patch is not None:
            assert patch.is_cuda and patch.dtype == torch.uint8 and patch.numel() >= n_batches * stride * 16
            d.d_patch = patch.data_ptr()
        if rw_state is not None:
            assert rw_state.is_cuda and rw_state.dtype == torch.uint8
            d.d_rw_state = rw_state.data_ptr()
        if ack_out is not None:   # INV launches: the ACK callbacks; ACK rows launches: the VAL callbacks, per row
            span = total if rows is None else (rows[0] - 1) * rows[1] + total
            assert unique and ack_out.is_cuda and ack_out.dtype == torch.uint8 and ack_out.numel() >= span * ack_out_size
            d.d_ack_out = ack_out.data_ptr()
            d.ack_out_size = int(ack_out_size)
        if offsets is not None:
            assert counts is None and offsets.is_cuda and offsets.dtype == torch.int32
            assert offsets.numel() >= n_batches + 1
            d.flags |= BATCH_PACKED
            d.d_counts = offsets.data_ptr()
        if counts is not None:
            assert counts.is_cuda and counts.dtype == torch.int32 and counts.numel() >= n_batches
            d.d_counts = counts.data_ptr()
        if rw is not None:
            assert rw.is_cuda and rw.dtype == torch.uint8
            d.d_rw = rw.data_ptr()
            d.rw_stride_bytes = int(rw_stride_bytes)
        if node_suspected is not None:
            assert node_suspected.is_cuda and node_suspected.dtype == torch.int32
            d.d_node_suspected = node_suspected.data_ptr()
        for i, b in enumerate(membership[:8]):
            d.membership[i] = b
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        self.launches += 1
        check(_L.hkv_batch_async(self.h, ctypes.byref(d), ctypes.c_void_p(s)), "hkv_batch_async")

    def batch_host(self, btype: int, elems: np.ndarray, membership: bytes, rw: np.ndarray | None = None,
                   n_batches: int = 1, stride: int | None = None, counts: np.ndarray | None = None,
                   rw_stride_elems: int = 0, node_suspected: np.ndarray | None = None,
                   offsets: np.ndarray | None = None, unique: bool = False) -> None:
        """Round-trip numpy arrays through the device path (parity tests). offsets: packed INV /
        VAL batches (HKV_BATCH_PACKED), batch b = elems[offsets[b]:offsets[b+1]]."""
        dev = torch.device("cuda", self.device)
        if offsets is not None:
            t = torch.from_numpy(elems.view(np.uint8).reshape(-1).copy()).to(dev)
            to = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).to(dev)
            tn = torch.from_numpy(np.ascontiguousarray(node_suspected, dtype=np.int32)).to(dev) \
                if node_suspected is not None else None
            tr = torch.from_numpy(rw.view(np.uint8).reshape(-1).copy()).to(dev) if rw is not None else None
            self.batch(btype, t, n_batches, len(elems), elems.dtype.itemsize, membership, rw=tr,
                       rw_stride_bytes=rw_stride_elems * (rw.dtype.itemsize if rw is not None else 0),
                       node_suspected=tn, offsets=to, unique=unique)
            torch.cuda.synchronize(dev)
            elems.view(np.uint8).reshape(-1)[:] = t.cpu().numpy()
            if rw is not None:
                rw.view(np.uint8).reshape(-1)[:] = tr.cpu().numpy()
            if node_suspected is not None:
                node_suspected[:] = tn.cpu().numpy()
            return
        stride = len(elems) // n_batches if stride is None else stride
        esz = elems.dtype.itemsize
        t = torch.from_numpy(elems.view(np.uint8).reshape(-1).copy()).to(dev)
        # local launches also keep the state mirror (d_state_out), checked against the elements
        local = int(btype) in (int(L.BatchType.local_ops), int(L.BatchType.local_ops_after_membership_change))
        st = torch.full((n_batches * stride,), 0xEE, dtype=torch.uint8, device=dev) if local else None
        tc = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev) if counts is not None else None
        tr = torch.from_numpy(rw.view(np.uint8).reshape(-1).copy()).to(dev) if rw is not None else None
        tn = torch.from_numpy(np.ascontiguousarray(node_suspected, dtype=np.int32)).to(dev) if node_suspected is not None else None
        self.batch(btype, t, n_batches, stride, esz, membership, tc, tr,
                   rw_stride_elems * (rw.dtype.itemsize if rw is not None else 0), tn, state_out=st, unique=unique)
        torch.cuda.synchronize(dev)
        elems.view(np.uint8).reshape(-1)[:] = t.cpu().numpy()
        if st is not None and not np.array_equal(st.cpu().numpy(),
                                                 elems.view(np.uint8).reshape(-1, esz)[: n_batches * stride, 9]):
            raise AssertionError("state mirror (d_state_out) differs from the elements' state bytes")
        if rw is not None:
            rw.view(np.uint8).reshape(-1)[:] = tr.cpu().numpy()
        if node_suspected is not None:
            node_suspected[:] = tn.cpu().numpy()

    def take_error_flags(self) -> int:
        """Internal-consistency flags raised by the device path since the last call (0 = none)."""
        v = ctypes.c_uint32(0)
        check(_L.hkv_take_error_flags(self.h, ctypes.byref(v)), "hkv_take_error_flags")
        return v.value

    def sync(self) -> None:
        check(_L.hkv_sync(self.h, None), "hkv_sync")

    # -- HBM image (reference byte layout)
    def index_bytes(self, offset: int = 0, nbytes: int | None = None) -> np.ndarray:
        nbytes = self.cfg.num_bkts * 64 - offset if nbytes is None else nbytes
        out = np.empty(nbytes, dtype=np.uint8)
        check(_L.hkv_copy_index(self.h, out.ctypes.data_as(ctypes.c_void_p), offset, nbytes), "hkv_copy_index")
        return out

    def log_bytes(self, offset: int = 0, nbytes: int | None = None) -> np.ndarray:
        nbytes = self.cfg.log_cap - offset if nbytes is None else nbytes
        out = np.empty(nbytes, dtype=np.uint8)
        check(_L.hkv_copy_log(self.h, out.ctypes.data_as(ctypes.c_void_p), offset, nbytes), "hkv_copy_log")
        return out

    def lookup_offset(self, key: int) -> int | None:
        """Log offset of a key's entry via the same 3-step lookup the batch path does."""
        key = int(key)
        bkt = (key & 0xFFFFFFFFFFFF) & (self.cfg.num_bkts - 1)
        slots = self.index_bytes(bkt * 64, 64).view("<u8")
        tag = key >> 48
        for s in slots:
            s = int(s)
            if (s & 1) and ((s >> 1) & 0x7FFFFF) == tag:
                off = s >> 24
                if self.log_head - off >= self.cfg.log_cap:
                    return None
                phys = off & (self.cfg.log_cap - 1)
                e = self.log_bytes(phys, 16).view("<u8")
                return phys if int(e[1]) == key else None
        return None

    def entry(self, key: int):
        off = self.lookup_offset(key)
        if off is None:
            return None
        return self.log_bytes(off, self.sizes.entry).view(L.entry_dtype(self.sizes))[0]

    # -- layouts (include/hermeskv.h, "Table layouts")
    def prefer_layout(self, layout: int) -> bool:
        """hkv_table_prefer_layout: the sticky preference; whether the table is eligible for it"""
        rc = _L.hkv_table_prefer_layout(self.h, int(layout))
        if rc < 0:
            check(rc, "hkv_table_prefer_layout")
        return rc == 1

    def layout(self) -> dict:
        """state, preference, eligibility and the counters (conversions, launches run while INLINE)"""
        v = HkvLayoutInfo()
        check(_L.hkv_table_layout(self.h, ctypes.byref(v)), "hkv_table_layout")
        return {"state": v.state, "preferred": v.preferred, "eligible": bool(v.eligible), "conversions": v.conversions,
                "inline_launches": v.inline_launches, "line_bytes": v.line_bytes}

    def apply_layout(self, stream: torch.cuda.Stream | None = None) -> None:
        """convert to the preferred layout now, as the next inline-capable launch would"""
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        check(_L.hkv_table_apply_layout(self.h, ctypes.c_void_p(s)), "hkv_table_apply_layout")

    def line_bytes(self, offset: int = 0, nbytes: int | None = None) -> np.ndarray:
        """debug export of the inline residency (128 B per bucket, private format)"""
        nbytes = self.cfg.num_bkts * 128 - offset if nbytes is None else nbytes
        out = np.empty(nbytes, dtype=np.uint8)
        check(_L.hkv_copy_lines(self.h, out.ctypes.data_as(ctypes.c_void_p), offset, nbytes), "hkv_copy_lines")
        return out

    # -- census (include/hermeskv.h, "Table census and digest")
    def census(self, stream: torch.cuda.Stream | None = None, offender_cap: int = 0,
               out: torch.Tensor | None = None, offender_keys: torch.Tensor | None = None) -> "Census":
        """hkv_table_census_async: the table's protocol state and digest, read in one pass from whichever
        residency the table is in (nothing is converted or exported), asynchronously on `stream` (default:
        torch's current). offender_cap: also list the keys of up to that many live keys that are not VALID.
        out / offender_keys: int64 device tensors to write into (CENSUS_WORDS words, overwritten; offender_cap
        keys or more, of which only the first min(offenders, offender_cap) are written) instead of new ones."""
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(CENSUS_WORDS, dtype=torch.int64, device=dev)
        assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= CENSUS_WORDS
        if offender_keys is None and offender_cap:
            offender_keys = torch.zeros(int(offender_cap), dtype=torch.int64, device=dev)
        if offender_keys is not None:
            assert offender_keys.is_cuda and offender_keys.dtype == torch.int64 and offender_keys.is_contiguous()
            assert offender_keys.numel() >= offender_cap
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        check(_L.hkv_table_census_async(self.h, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(offender_keys.data_ptr()) if offender_cap else None,
                                        int(offender_cap), ctypes.c_void_p(s)), "hkv_table_census_async")
        return Census(out[:CENSUS_WORDS], offender_keys[:offender_cap] if offender_cap else None)

    def census_host(self) -> dict:
        """hkv_table_census: the same, synchronous, as a dict (no offender list)"""
        v = HkvCensus()
        check(_L.hkv_table_census(self.h, ctypes.byref(v)), "hkv_table_census")
        return _census_dict(bytes(v))

    def census_parts(self, part_bits: int, out: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None) -> "PartRows":
        """hkv_table_census_parts_async: the census's digest_sum, digest_xor, keys and not-VALID count per partition
        p = key & (2^part_bits - 1) of the live keys, as PartRows ([P, 4] int64 on the device, no host read), read
        in one pass from whichever residency the table is in (nothing is converted), asynchronously on `stream`
        (default: torch's current). part_bits <= log2(num_bkts), so that every key of a bucket lies in one partition;
        a larger value is refused. The rows fold to census(): sums add, digest_xor xors. Equal tables, of any bucket
        count, log order or residency, give equal rows. out: a contiguous int64 device tensor of 4 * 2^part_bits
        words or more to write into (overwritten) instead of a new one. Tables with RMWs are accepted."""
        part_bits = int(part_bits)
        if not 0 <= part_bits < int(self.cfg.num_bkts).bit_length():
            # more partitions than buckets: the library's refusal (it launches nothing), before 2^part_bits rows
            # are asked of the allocator
            row = torch.empty(4, dtype=torch.int64, device=torch.device("cuda", self.device))
            check(_L.hkv_table_census_parts_async(self.h, part_bits & 0xFFFFFFFF, ctypes.c_void_p(row.data_ptr()),
                                                  None), "hkv_table_census_parts_async")
            raise HkvError(f"hkv_table_census_parts_async: part_bits {part_bits}")
        P = 1 << part_bits
        if out is None:
            out = torch.empty(P * 4, dtype=torch.int64, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= P * 4
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        check(_L.hkv_table_census_parts_async(self.h, int(part_bits), ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(s)), "hkv_table_census_parts_async")
        return PartRows(out.view(-1)[:P * 4].view(P, 4), int(part_bits))

    # -- replica repair (include/hermeskv.h, "Replica repair")
    def extract(self, bkt_range: tuple[int, int] | None = None, min_ts: int = 0, out: torch.Tensor | None = None,
                cap: int | None = None, stream: torch.cuda.Stream | None = None,
                result: torch.Tensor | None = None, part_bits: int | None = None,
                part_mask: torch.Tensor | None = None) -> "Extract":
        """hkv_table_extract_async: one record per live key of the buckets bkt_range = (lo, hi) (default: all) whose
        packed timestamp (version << 8 | cid) is at least min_ts, read from whichever residency the table is in
        (nothing is converted), asynchronously on `stream` (default: torch's current). out: a uint8 device buffer
        to write into (its whole records are the capacity) instead of a new one of `cap` records (default: the
        table's num_keys); result: two int64 words to write the counts into. Records past the capacity are counted,
        not written. min_ts only saves volume: the protocol has no global watermark, so whether the keys it leaves
        out are current at the target is the caller's to know. Not for tables with RMWs.
        part_bits, part_mask (both or neither; None: the call above, unchanged): hkv_table_extract_parts_async --
        only the buckets whose partition b & (2^part_bits - 1) has a non-zero byte in part_mask (uint8 device
        tensor, 2^part_bits bytes; part_bits <= log2(num_bkts)) are read, and scanned_keys counts those alone."""
        dev = torch.device("cuda", self.device)
        E = self.sizes.entry
        assert (part_bits is None) == (part_mask is None), "part_bits and part_mask go together"
        if out is None:
            out = torch.empty(max(int(self.num_keys if cap is None else cap), 1) * E, dtype=torch.uint8, device=dev)
            n_cap = int(self.num_keys if cap is None else cap)
        else:
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
            n_cap = out.numel() // E if cap is None else int(cap)
            assert n_cap * E <= out.numel()
        if result is None:
            result = torch.empty(2, dtype=torch.int64, device=dev)
        assert result.is_cuda and result.dtype == torch.int64 and result.is_contiguous() and result.numel() >= 2
        lo, hi = (0, self.cfg.num_bkts) if bkt_range is None else (int(bkt_range[0]), int(bkt_range[1]))
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        if part_mask is not None:
            assert part_mask.is_cuda and part_mask.dtype == torch.uint8 and part_mask.is_contiguous()
            assert part_mask.numel() >= 1 << int(part_bits)
            check(_L.hkv_table_extract_parts_async(self.h, int(part_bits), ctypes.c_void_p(part_mask.data_ptr()), lo, hi,
                                                   int(min_ts), ctypes.c_void_p(out.data_ptr()), n_cap,
                                                   ctypes.c_void_p(result.data_ptr()), ctypes.c_void_p(s)),
                  "hkv_table_extract_parts_async")
            return Extract(out[:n_cap * E], result[:2], E)
        check(_L.hkv_table_extract_async(self.h, lo, hi, int(min_ts), ctypes.c_void_p(out.data_ptr()), n_cap,
                                         ctypes.c_void_p(result.data_ptr()), ctypes.c_void_p(s)),
              "hkv_table_extract_async")
        return Extract(out[:n_cap * E], result[:2], E)

    def install(self, records, n: int | None = None, stream: torch.cuda.Stream | None = None,
                result: torch.Tensor | None = None) -> "InstallResult":
        """hkv_table_install_async: apply n records (an Extract, or a uint8 device tensor of whole records), no key
        twice among them, as the reference would apply one INV per record (sender = the record's ts cid) and then
        one VAL per record whose source state was VALID: newer records install value, timestamp and state, equal
        ones touch what an INV and a VAL of that timestamp touch, older ones nothing, unknown keys are misses.
        n omitted: for an Extract min(records, capacity), which is read on the host (a synchronisation: pass n to
        stay on the stream); for a tensor, all its whole records. Asynchronous on `stream`. A repair is sound
        while this table takes no client operations; INVs it receives meanwhile are safe, the install being
        timestamp-guarded. Re-admission to the membership is not part of it. Not for tables with RMWs."""
        E = self.sizes.entry
        t = records.tensor if isinstance(records, Extract) else records
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        if n is None:
            n = records.written if isinstance(records, Extract) else t.numel() // E
        n = int(n)
        assert 0 <= n and n * E <= t.numel()
        if result is None:
            result = torch.empty(4, dtype=torch.int64, device=t.device)
        assert result.is_cuda and result.dtype == torch.int64 and result.is_contiguous() and result.numel() >= 4
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        self.launches += 1
        check(_L.hkv_table_install_async(self.h, ctypes.c_void_p(t.data_ptr()), n, ctypes.c_void_p(result.data_ptr()),
                                         ctypes.c_void_p(s)), "hkv_table_install_async")
        return InstallResult(result[:4])

    # -- upsert (include/hermeskv.h, "Upsert")
    def upsert(self, records, n: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
        """hkv_table_upsert: install() of the n records (an Extract, or a uint8 device tensor of whole records, no
        key twice among them) and then, for every record the install missed, in record order, the reference's
        insert (mica_insert_one) of the entry that record stands for. Returns hkv_upsert_result as a dict: raised,
        equal, older (the install's counts), inserted (its missed), replaced (inserts that took an in-use slot by
        tag match: the key that slot led to is lost), evictions (inserts that found no slot) and log_head. Unlike
        install() the call returns when its work on `stream` is done: the number of inserts is known only on the
        device and the log head lives on the host. With nothing missed it is an install (an INLINE table stays
        INLINE); otherwise the table goes to LOG first, as before a populate. num_keys follows the inserts, so a
        later extract()'s default buffer holds them. Not for tables with RMWs."""
        E = self.sizes.entry
        t = records.tensor if isinstance(records, Extract) else records
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        if n is None:
            n = records.written if isinstance(records, Extract) else t.numel() // E
        n = int(n)
        assert 0 <= n and n * E <= t.numel()
        out = HkvUpsertResult()
        if n == 0:   # (an empty tensor has no address to pass)
            return {name: self.log_head if name == "log_head" else 0 for name, _ in HkvUpsertResult._fields_[:7]}
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        self.launches += 1
        check(_L.hkv_table_upsert(self.h, ctypes.c_void_p(t.data_ptr()), n, ctypes.byref(out), ctypes.c_void_p(s)),
              "hkv_table_upsert")
        self.num_keys += int(out.inserted)
        return {name: int(getattr(out, name)) for name, _ in HkvUpsertResult._fields_[:7]}

    # -- key-level delta repair (include/hermeskv.h, "Key-level delta repair")
    def summaries(self, bkt_range: tuple[int, int] | None = None, min_ts: int = 0, part_bits: int | None = None,
                  part_mask: torch.Tensor | None = None, out: torch.Tensor | None = None, cap: int | None = None,
                  stream: torch.cuda.Stream | None = None) -> "Summaries":
        """hkv_table_summaries_async: one 16-byte summary (key, ts version, ts cid, state) per live key that
        extract() with the same bkt_range, min_ts, part_bits and part_mask would emit a record for, compacted in no
        particular order, read from whichever residency the table is in (nothing is converted), asynchronously on
        `stream` (default: torch's current). part_mask None: every partition (part_bits then defaults to 0).
        out: a uint8 device buffer to write into (its whole summaries are the capacity) instead of a new one of
        `cap` summaries (default: the table's num_keys). Summaries past the capacity are counted, not written.
        Read-only; not for tables with RMWs."""
        dev = torch.device("cuda", self.device)
        part_bits = 0 if part_bits is None else int(part_bits)
        if out is None:
            n_cap = int(self.num_keys if cap is None else cap)
            out = torch.empty(max(n_cap, 1) * SUMMARY_BYTES, dtype=torch.uint8, device=dev)
        else:
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
            n_cap = out.numel() // SUMMARY_BYTES if cap is None else int(cap)
            assert n_cap * SUMMARY_BYTES <= out.numel()
        result = torch.empty(2, dtype=torch.int64, device=dev)
        lo, hi = (0, self.cfg.num_bkts) if bkt_range is None else (int(bkt_range[0]), int(bkt_range[1]))
        if part_mask is not None:
            assert part_mask.is_cuda and part_mask.dtype == torch.uint8 and part_mask.is_contiguous()
            assert part_bits >= 64 or part_mask.numel() >= 1 << part_bits
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        check(_L.hkv_table_summaries_async(self.h, part_bits & 0xFFFFFFFF,
                                           ctypes.c_void_p(part_mask.data_ptr()) if part_mask is not None else None,
                                           lo, hi, int(min_ts), ctypes.c_void_p(out.data_ptr()), n_cap,
                                           ctypes.c_void_p(result.data_ptr()), ctypes.c_void_p(s)),
              "hkv_table_summaries_async")
        return Summaries(out[:n_cap * SUMMARY_BYTES], result, SUMMARY_BYTES)

    def need(self, summaries, n: int | None = None, out: torch.Tensor | None = None,
             stream: torch.cuda.Stream | None = None) -> "Need":
        """hkv_table_need_async: look the n summaries up (a Summaries, or a contiguous uint8 / int64 device tensor
        of whole summaries) and class each against this table's entry: missed, newer, validate (equal timestamp,
        the summary VALID, the entry not), same, state_only, older. A key is needed exactly when installing its
        record would miss or change a byte the digest keeps: missed, newer and validate. Returns a Need: the needed
        keys compacted (int64, no particular order; `out`: a tensor to write them into, whose length is the
        capacity, instead of a new one of n) and the seven counts, all still on the device. n omitted: for a
        Summaries min(records, capacity), read on the host (pass n to stay on the stream); for a tensor, all of
        it. Nothing is written to the table; duplicates among the summaries are harmless. Not for tables with RMWs."""
        t = summaries.tensor if isinstance(summaries, Summaries) else summaries
        assert t.is_cuda and t.dtype in (torch.uint8, torch.int64) and t.is_contiguous()
        if n is None:
            n = summaries.written if isinstance(summaries, Summaries) else t.numel() * t.element_size() // SUMMARY_BYTES
        n = int(n)
        assert 0 <= n and n * SUMMARY_BYTES <= t.numel() * t.element_size()
        if out is None:
            out = torch.empty(max(n, 2), dtype=torch.int64, device=t.device)
            need_cap = n
        else:
            assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous()
            need_cap = out.numel()
        result = torch.empty(8, dtype=torch.int64, device=t.device)
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        check(_L.hkv_table_need_async(self.h, ctypes.c_void_p(t.data_ptr()) if n else None, n,
                                      ctypes.c_void_p(out.data_ptr()) if need_cap else None, need_cap,
                                      ctypes.c_void_p(result.data_ptr()), ctypes.c_void_p(s)), "hkv_table_need_async")
        return Need(out[:need_cap], result[:7])

    def fetch(self, keys, n: int | None = None, out: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None) -> "Fetch":
        """hkv_table_fetch_async: the records of n keys (a Need, or a contiguous int64 device tensor), by position:
        record i is key i's, in extract()'s record format, read from whichever residency the table is in (nothing
        is converted). A key the table does not hold gives a record that is zero but for its key bytes and counts
        as absent; a key may repeat. out: a uint8 device buffer of n * E bytes or more to write into instead of a
        new one. n omitted: for a Need min(needed, capacity), read on the host; for a tensor, all of it. Read-only;
        not for tables with RMWs."""
        E = self.sizes.entry
        t = keys.keys if isinstance(keys, Need) else keys
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
        if n is None:
            n = keys.written if isinstance(keys, Need) else t.numel()
        n = int(n)
        assert 0 <= n <= t.numel()
        if out is None:
            out = torch.empty(max(n, 1) * E, dtype=torch.uint8, device=t.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n * E
        result = torch.empty(2, dtype=torch.int64, device=t.device)
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        check(_L.hkv_table_fetch_async(self.h, ctypes.c_void_p(t.data_ptr()) if n else None, n,
                                       ctypes.c_void_p(out.data_ptr()) if n else None,
                                       ctypes.c_void_p(result.data_ptr()), ctypes.c_void_p(s)), "hkv_table_fetch_async")
        return Fetch(out[:n * E], result, E)

    def device_index(self) -> int:
        return _L.hkv_device_index(self.h)

    def device_log(self) -> int:
        return _L.hkv_device_log(self.h)


def hash_ids(ids: torch.Tensor, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """CityHash128(&id, 4).second for each uint32 id, on the GPU (mica_gen_keys)."""
    assert ids.is_cuda and ids.dtype == torch.int32
    out = torch.empty(ids.numel(), dtype=torch.int64, device=ids.device)
    s = (stream or torch.cuda.current_stream(ids.device)).cuda_stream
    check(_L.hkv_hash_ids(ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(out.data_ptr()), ids.numel(),
                          ctypes.c_void_p(s)), "hkv_hash_ids")
    return out


# ---------------------------------------------------------------- sketch-level delta repair
SKETCH_CELL_BYTES = 32   # hkv_sketch_cell: count, key_xor, meta_xor, check_xor
SKETCH_MAX_PASSES = 192  # HKV_SKETCH_MAX_PASSES
SKETCH_FIELDS = ("only_a", "only_b", "undecoded", "passes", "exhausted")   # hkv_sketch_result's first five words


def _u64(x) -> int:
    return int(x) & 0xFFFFFFFFFFFFFFFF


@dataclasses.dataclass
class Sketch:
    """The result of sketch(), still on the device. `cells`: int64[3 * sub_cells, 4], cell i = hkv_sketch_cell
    (count, key_xor, meta_xor, check_xor: the unsigned words' bit patterns) of include/hermeskv.h "Sketch-level
    delta repair"; subtable j is rows [j * sub_cells, (j + 1) * sub_cells). host() synchronises."""
    cells: torch.Tensor
    sub_cells: int

    @property
    def nbytes(self) -> int:
        return 3 * self.sub_cells * SKETCH_CELL_BYTES

    def host(self) -> np.ndarray:
        """the cells as uint64 [3 * sub_cells, 4]"""
        return self.cells.cpu().numpy().view(np.uint64)


@dataclasses.dataclass
class SketchDecode:
    """The result of sketch_decode(), still on the device. `only_a`, `only_b`: uint8 buffers of cap_a, cap_b
    16-byte summaries, of which the first min(count, cap) are the elements taken, in no particular order;
    `result`: hkv_sketch_result as eight int64 words; `remainder`: the Sketch that went in as `a`, now holding the
    2-core. host(), the attributes named in SKETCH_FIELDS, only_a_host() and only_b_host() synchronise."""
    only_a: torch.Tensor
    only_b: torch.Tensor
    result: torch.Tensor
    remainder: Sketch

    def host(self) -> dict:
        return {k: _u64(x) for k, x in zip(SKETCH_FIELDS, self.result.cpu().tolist())}

    def __getattr__(self, name: str):
        if name in SKETCH_FIELDS:
            return self.host()[name]
        raise AttributeError(name)

    def _list_host(self, buf: torch.Tensor, count: int) -> np.ndarray:
        n = min(count, buf.numel() // SUMMARY_BYTES)
        return buf[:n * SUMMARY_BYTES].cpu().numpy().view(SUMMARY_DTYPE)

    def only_a_host(self) -> np.ndarray:
        """the summaries only `a` held, min(only_a, cap_a) of them as a SUMMARY_DTYPE array"""
        return self._list_host(self.only_a, self.host()["only_a"])

    def only_b_host(self) -> np.ndarray:
        """the summaries only `b` held, min(only_b, cap_b) of them as a SUMMARY_DTYPE array"""
        return self._list_host(self.only_b, self.host()["only_b"])


def sketch(summaries, sub_cells: int, n: int | None = None, out: "Sketch | torch.Tensor | None" = None,
           accumulate: bool = False, stream: torch.cuda.Stream | None = None) -> Sketch:
    """hkv_summaries_sketch_async: fold n 16-byte summaries (a Summaries, or a contiguous uint8 / int64 device
    tensor of whole summaries) into an invertible sketch of 3 * sub_cells cells (include/hermeskv.h "Sketch-level
    delta repair"), asynchronously on `stream` (default: torch's current). The cells are a function of the multiset
    of summaries, so equal lists give equal bytes in whatever order. out: a Sketch of the same sub_cells, or an
    int64 device tensor of 3 * sub_cells * 4 words, to fold into instead of a new one; accumulate: add to what `out`
    holds instead of overwriting it. n omitted: for a Summaries min(records, capacity), read on the host (pass n to
    stay on the stream); for a tensor, all of it."""
    t = summaries.tensor if isinstance(summaries, Summaries) else summaries
    assert t.is_cuda and t.dtype in (torch.uint8, torch.int64) and t.is_contiguous()
    if n is None:
        n = summaries.written if isinstance(summaries, Summaries) else t.numel() * t.element_size() // SUMMARY_BYTES
    n, S = int(n), int(sub_cells)
    assert 0 <= n and n * SUMMARY_BYTES <= t.numel() * t.element_size()
    if out is None:
        assert not accumulate, "accumulate adds to the cells of `out`"
        cells = torch.empty((3 * S, 4), dtype=torch.int64, device=t.device)
    else:
        cells = out.cells if isinstance(out, Sketch) else out
        assert cells.is_cuda and cells.dtype == torch.int64 and cells.is_contiguous() and cells.numel() == 12 * S
        cells = cells.view(3 * S, 4)
    with torch.cuda.device(t.device):
        s = (stream or torch.cuda.current_stream(t.device)).cuda_stream
        check(_L.hkv_summaries_sketch_async(ctypes.c_void_p(t.data_ptr()) if n else None, n,
                                            ctypes.c_void_p(cells.data_ptr()), S, int(bool(accumulate)),
                                            ctypes.c_void_p(s)), "hkv_summaries_sketch_async")
    return Sketch(cells, S)


def sketch_decode(a: Sketch, b: Sketch, cap_a: int | None = None, cap_b: int | None = None,
                  stream: torch.cuda.Stream | None = None) -> SketchDecode:
    """hkv_sketch_decode_async: subtract sketch `b` from sketch `a` (same sub_cells) and peel the difference. `a`
    is overwritten: it ends as the remainder (all zero when the decode is complete). Returns a SketchDecode, still
    on the device: the summaries only `a` held and those only `b` held (buffers of cap_a / cap_b summaries, default
    3 * sub_cells each, which no decode can exceed by more than duplicates; counts past a cap are counted, not
    written) and the result words (only_a, only_b, undecoded, passes, exhausted). Every kernel is enqueued up
    front on `stream` (default: torch's current); nothing is read back until a count is asked for."""
    assert a.sub_cells == b.sub_cells and a.cells.device == b.cells.device, "two sketches of one sub_cells"
    assert a.cells.data_ptr() != b.cells.data_ptr()
    S, dev = a.sub_cells, a.cells.device
    cap_a = 3 * S if cap_a is None else int(cap_a)
    cap_b = 3 * S if cap_b is None else int(cap_b)
    la = torch.empty(max(cap_a, 1) * SUMMARY_BYTES, dtype=torch.uint8, device=dev)
    lb = torch.empty(max(cap_b, 1) * SUMMARY_BYTES, dtype=torch.uint8, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        s = (stream or torch.cuda.current_stream(dev)).cuda_stream
        check(_L.hkv_sketch_decode_async(ctypes.c_void_p(a.cells.data_ptr()), ctypes.c_void_p(b.cells.data_ptr()), S,
                                         ctypes.c_void_p(la.data_ptr()) if cap_a else None, cap_a,
                                         ctypes.c_void_p(lb.data_ptr()) if cap_b else None, cap_b,
                                         ctypes.c_void_p(result.data_ptr()), ctypes.c_void_p(s)),
              "hkv_sketch_decode_async")
    return SketchDecode(la[:cap_a * SUMMARY_BYTES], lb[:cap_b * SUMMARY_BYTES], result, a)
