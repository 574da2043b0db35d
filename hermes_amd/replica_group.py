"""A Hermes replica group with one replica per GPU.

Hermes replicates every key on every node, so N GPUs form an N-replica group (N <= 8: the
membership bit vectors are 8 bits wide, spacetime.h:188-195). The wings RDMA layer
(wings.h:770-916) becomes three data collectives per protocol round, on torch's current stream:

  1. every replica packs the round's INVs (at most C per worker: the send credits) into one
     contiguous slab, worker after worker; the totals are all-gathered and the host reads the
     largest, the round's width (the one host synchronisation of a round). The INV slabs are
     all-gathered as [N][width] x op_size
  2. every replica applies its peers' INVs as one INV batch launch of N batches (one per peer,
     its own masked out by a zero count); the ACKs (INV-aborts with RMWs) are written in the
     positions of the INVs they answer and go back to the coordinators with an all-to-all:
     row p of the ACK slab holds rank p's ACKs, lined up with the slab rank p sent
  3. coordinators regroup the ACKs per worker through their own packing offsets (one receive
     poll over all peers), apply them as an ACK batch against the worker's op buffer
     (read_write_ops), pack the VALs of the writes that completed and all-gather them at the
     same width (a round completes at most the writes it INV'd); every replica applies its
     peers' VALs as one VAL batch.

Packed slabs carry what a round sends, not the credits' worst case: at 20 % writes about 24 INVs
per worker go out, against C = 104 slots, so the collectives and the INV/VAL launches are about
4x smaller than with [N][W][C] rows. `ReplicaRound` holds one replica's buffers and phases;
`ReplicaGroupRound` drives one replica per process over torch.distributed (RCCL);
`LoopbackGroup` drives N replicas in one process (tests: the same phases and kernels, with the
collectives done by tensor copies).
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import layout as L
from .kvs import HermesKV
from .lib import check, raw
from .hades import NO_VIEW, Hades, MajorityLost, exchange_views
from .workload import HkvZipf, _ptr, _s, init_mirrors, refill_flags, slots_per_worker  # noqa: F401 (re-exported)

_L = raw()
_P = ctypes.c_void_p
_L.hkv_wl_marshal_acks_rows.argtypes = [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P,
                                        ctypes.c_uint32, _P, ctypes.c_uint32, _P]
_L.hkv_wl_regroup.argtypes = [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P,
                              ctypes.c_int32, _P, _P]
_L.hkv_wl_collect_vals.argtypes = [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P, ctypes.c_int32,
                                   _P, ctypes.c_uint32, _P, _P, _P]
_L.hkv_wl_fold_counters.argtypes = [_P, _P]
_L.hkv_wl_pack_rows.argtypes = [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P, _P, _P]
_L.hkv_wl_marshal_acks_aligned.argtypes = [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P,
                                           ctypes.c_uint32, ctypes.c_uint32, _P]
_L.hkv_wl_marshal_memb_vals.argtypes = [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P, ctypes.c_int32, _P,
                                        ctypes.c_uint32, _P, _P]
_L.hkv_wl_regroup_aligned.argtypes = [_P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_int32, ctypes.c_uint32,
                                      _P, ctypes.c_int32, _P, _P]
_L.hkv_wl_marshal_invs_packed.argtypes = [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _P, ctypes.c_int32,
                                          ctypes.c_int32, _P, _P, _P, _P, ctypes.c_uint32, _P, _P]
_L.hkv_wl_collect_vals_rows.argtypes = [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, _P,
                                        ctypes.c_int32, _P, ctypes.c_uint32, _P, _P, _P]

MAX_REPLICAS = 8
LOCAL = 250  # MAX_BATCH_KVS_OPS_SIZE, config.h:42


class ReplicaRound:
    """Buffers and phases of one replica (machine id = rank) of an N-replica group."""

    def __init__(self, kvs: HermesKV, n_workers: int, world: int, rank: int, zipf: HkvZipf,
                 write_permille: int = 200, rmw_permille: int = 0, seed: int = 0x5EED,
                 trace_len: int = 8192, retry_stalled: bool = False, slots: int | None = None,
                 fused_refill: bool = True):
        if not 2 <= world <= MAX_REPLICAS:
            raise ValueError(f"a replica group has 2..{MAX_REPLICAS} replicas, got {world}")
        if kvs.machine_id != rank:
            raise ValueError("the replica's table must use machine_id == rank")
        self.kvs, self.W, self.N, self.rank = kvs, n_workers, world, rank
        self.sizes = kvs.sizes
        self.op = kvs.sizes.op
        self.ack_size = self.op if kvs.rmw else L.OP_META_SIZE
        self.mb = L.membership(world, rank)
        self.retry = retry_stalled
        self.rflags = refill_flags(kvs, retry_stalled)
        self.C = slots or slots_per_worker(write_permille, rmw_permille)
        W, N, C = n_workers, world, self.C
        dev = torch.device("cuda", kvs.device)
        u8 = dict(dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ops = torch.zeros(W * LOCAL * self.op, **u8)
        self.states = torch.zeros(W * LOCAL, dtype=torch.uint8, device=dev)  # local batch state mirror
        self.opcodes = torch.zeros(W * LOCAL, dtype=torch.uint8, device=dev)  # the refill's opcode mirror
        # refills planned from the state mirror and applied by the next local launch (workload.Round)
        self.fused = fused_refill and self.op <= 64
        self.patch = torch.zeros(W * LOCAL * 16, **u8) if self.fused else None
        # outgoing INVs: [W][C] rows, then packed (worker w at inv_off[w]; inv_off[W] = total)
        self.inv_count = torch.zeros(W, **i32)           # INVs each worker sends this round
        self.inv_sendable = torch.zeros(W, **i32)        # ... and could send (the rest are held)
        self.inv_off = torch.zeros(W + 1, **i32)
        # the INVs go straight into the packed slab, at most `cap` per rank and round (local(cap)), so the
        # group can size its collectives without a host read
        self.packed_marshal = True
        self.inv_pack = torch.zeros(W * C * self.op, **u8)
        self.inv_totals = torch.zeros(N, **i32)          # all ranks' INV totals (this round's width: max)
        self.inv_maxc = torch.zeros(1, **i32)            # this rank's largest per-worker INV count
        # receive buffers at the largest width (W * C); a round uses [N][width] of them
        self.inv_recv = torch.zeros(N * W * C * self.op, **u8)
        self.ack_slab = torch.zeros(N * W * C * self.ack_size, **u8)
        self.ack_recv = torch.zeros(N * W * C * self.ack_size, **u8)
        self.ack_batch = torch.zeros(W * N * C * self.ack_size, **u8)
        self.ack_batch_count = torch.zeros(W, **i32)
        self.val_slab = torch.zeros(W * C * L.OP_META_SIZE, **u8)
        self.val_count = torch.zeros(W, **i32)
        self.val_off = torch.zeros(W + 1, **i32)
        self.val_pack = torch.zeros(W * C * L.OP_META_SIZE, **u8)
        self.val_totals = torch.zeros(N, **i32)
        self.val_recv = torch.zeros(N * W * C * L.OP_META_SIZE, **u8)
        self.held = torch.zeros(2, dtype=torch.int64, device=dev)    # INVs held back, VALs dropped
        self.cursor = torch.zeros(W, **i32)
        self.counters = torch.zeros(4096, dtype=torch.int64, device=dev)  # HKV_WL_COUNTER_WORDS
        self.inv_total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.elem_totals = torch.zeros(3, dtype=torch.int64, device=dev)  # INV, ACK, VAL elements applied
        self.count_elems = True        # keep inv_total / elem_totals (small torch ops per phase)
        self.trace_len = trace_len
        self.trace_key = torch.empty(W * trace_len, dtype=torch.int64, device=dev)
        self.trace_op = torch.empty(W * trace_len, **u8)
        check(_L.hkv_wl_gen_trace(_ptr(self.trace_key), _ptr(self.trace_op), None, W, trace_len,
                                  ctypes.byref(zipf), write_permille, rmw_permille,
                                  ctypes.c_uint64(seed ^ (rank << 48)), _s()), "gen_trace")
        self.failed = False            # this replica has failed (fail()): it sends nothing more
        # ACK rows applied as they arrive, one unique-key launch per peer (a peer answers each of this
        # replica's INVs once, and a key has one local write in flight), with no regroup pass; once any
        # replica has failed, its rows hold empty slots and the regrouped batch takes over for good
        self.unique_acks = True
        # ... all peers' rows in one launch (HKV_BATCH_ROWS, this rank's own row skipped; 64-B entries and
        # 16-B ACKs, otherwise one launch per peer)
        self.ack_rows = self.sizes.entry == 64 and self.ack_size <= 64
        self.own_total = None          # this round's packed INV total, when read back (round_shape)
        # this replica's ACKs to a peer's INVs written by that peer's INV launch itself (hkv_batch_desc.d_ack_out,
        # as at N = 1) instead of a marshal pass over the applied row
        self.fused_acks = (self.sizes.entry == 64 and self.op <= 64) or (self.sizes.entry == 320 and self.op <= 320)
        self.refill(first=True)

    # -- Hades: one view-update period per round when enabled
    def hades_start(self):
        self.hades = Hades(self.N, self.rank)

    def hades_row(self, changed: bool) -> bytes:
        """this replica's heartbeats (one 4-byte view per destination) and a 4-byte trailer:
        [membership changed this period, membership is the whole group]; a failed replica sends
        nothing"""
        if self.failed:
            return bytes([NO_VIEW, 0, 0, 0]) * self.N + bytes(4)
        g, _ = self.hades.state()
        return self.hades.views_row() + bytes([int(changed), int(g == (1 << self.N) - 1), 0, 0])

    # -- phases (all asynchronous on torch's current stream)
    def fail(self):
        """This replica fails after its INVs of the current round went out: from now on it sends
        no ACKs, VALs or INVs (it still joins the collectives, with empty slabs)."""
        self.failed = True
        self.unique_acks = False

    def peer_failing(self):
        """Some replica fails this round: its ACK rows hold empty slots from now on"""
        self.unique_acks = False

    def refill(self, first: bool = False):
        if self.failed:
            return
        if self.fused and not first:
            check(_L.hkv_wl_refill_plan(_ptr(self.states), self.W, LOCAL, self.sizes.st_value, self.sizes.shift,
                                        _ptr(self.trace_key), _ptr(self.trace_op), self.trace_len, _ptr(self.cursor),
                                        self.rank, self.rflags, _ptr(self.counters), _ptr(self.opcodes),
                                        _ptr(self.patch), _s()), "refill_plan")
            return
        check(_L.hkv_wl_refill(_ptr(self.ops), self.W, LOCAL, self.op, self.sizes.st_value, self.sizes.shift,
                               _ptr(self.trace_key), _ptr(self.trace_op), None, self.trace_len, _ptr(self.cursor),
                               self.rank, int(first), self.rflags, _ptr(self.counters), _ptr(self.opcodes), None,
                               _s()), "refill")
        if first:
            init_mirrors(self.ops, self.op, self.states)

    def local(self, cap: int | None = None):
        """Local batch, then this round's INVs, packed (inv_pack; worker w at inv_off[w]); at most `cap` of
        them (the rest keep their state and go out in a later round, counted in held[0])."""
        if self.failed:
            self.inv_count.zero_()
            self.inv_off.zero_()
            self.inv_maxc.zero_()
            return
        self.kvs.batch(L.BatchType.local_ops, self.ops, self.W, LOCAL, self.op, self.mb, state_out=self.states,
                       opcode_in=self.opcodes, patch=self.patch)
        check(_L.hkv_wl_marshal_invs_packed(_ptr(self.ops), self.W, LOCAL, self.op, _ptr(self.states), self.C,
                                            self.W * self.C if cap is None else int(cap), _ptr(self.inv_pack),
                                            _ptr(self.inv_off), _ptr(self.inv_sendable), _ptr(self.inv_count),
                                            self.rank, _ptr(self.held), _s()), "marshal_invs_packed")
        torch.amax(self.inv_count, dim=0, keepdim=True, out=self.inv_maxc)
        if self.count_elems:
            self.inv_total += self.inv_off[self.W]

    # -- the slabs each collective moves: (receive, send) views at the round's width
    def inv_total_io(self):
        return self.inv_totals, self.inv_off[self.W:]

    def round_shape(self) -> tuple[int, int]:
        """After the totals are gathered (host synchronisation): the round's width (the largest
        INV total of any rank) and this rank's ACK batch stride ((N-1) x its largest per-worker
        INV count: a worker gets at most one ACK per INV from every peer). Also keeps this rank's
        own INV total (own_total) for the per-peer ACK launches."""
        v = torch.cat([self.inv_totals.max().view(1), self.inv_maxc, self.inv_off[self.W:]]).cpu().tolist()
        self.own_total = int(v[2])
        return max(1, int(v[0])), max(1, (self.N - 1) * int(v[1]))

    def inv_io(self, width: int):
        n = width * self.op
        return self.inv_recv[:self.N * n], self.inv_pack[:n]

    def ack_io(self, width: int):
        n = self.N * width * self.ack_size
        return self.ack_recv[:n], self.ack_slab[:n]

    def val_total_io(self):
        return self.val_totals, self.val_off[self.W:]

    def val_io(self, width: int):
        n = width * L.OP_META_SIZE
        return self.val_recv[:self.N * n], self.val_pack[:n]

    # steady rounds (WidthPlan): each slab is one slot wider than the INV cap and carries its rank's
    # total in that spare slot, so the totals travel with the slabs (two collectives per round fewer)
    def _put_total(self, pack, width: int, size: int, off) -> None:
        a = (width - 1) * size
        pack[a:a + 4].view(torch.int32).copy_(off[self.W:])

    def _take_totals(self, recv, width: int, size: int, out) -> None:
        a = (width - 1) * size
        out.copy_(recv[:self.N * width * size].view(self.N, width * size)[:, a:a + 4].view(torch.int32).view(-1))

    def inv_io_total(self, width: int):
        """inv_io, the spare slot (width - 1) of the send slab holding this rank's INV total"""
        self._put_total(self.inv_pack, width, self.op, self.inv_off)
        return self.inv_io(width)

    def take_inv_totals(self, width: int) -> None:
        """inv_totals from the spare slots of the gathered INV slabs"""
        self._take_totals(self.inv_recv, width, self.op, self.inv_totals)

    def val_io_total(self, width: int):
        self._put_total(self.val_pack, width, L.OP_META_SIZE, self.val_off)
        return self.val_io(width)

    def take_val_totals(self, width: int) -> None:
        self._take_totals(self.val_recv, width, L.OP_META_SIZE, self.val_totals)

    def invs(self, width: int):
        """Apply the gathered INVs of the peers ([N][width], row p: inv_totals[p] INVs) as N
        batches; their ACKs go into ack_slab in the positions of the INVs they answer."""
        self.inv_totals[self.rank:self.rank + 1].zero_()   # (an indexed store from the host would synchronise)
        if self.failed:   # no ACKs from a failed replica
            self.ack_slab[:self.N * width * self.ack_size].view(-1, self.ack_size)[:, 8] = int(L.Bucket.EMPTY)
            return
        if self.count_elems:
            self.elem_totals[0] += self.inv_totals.sum()
        # one launch per peer, in rank order: a peer's slab holds at most one INV per key (one write in
        # flight per key and coordinator), so each applies in one pass (HKV_BATCH_UNIQUE)
        for p in range(self.N):
            if p != self.rank:
                self._inv_launch(p, width)
        if not self.fused_acks:
            check(_L.hkv_wl_marshal_acks_aligned(_ptr(self.inv_recv), _ptr(self.inv_totals), self.N, width, self.op,
                                                 _ptr(self.ack_slab), self.ack_size, self.rank, _s()), "marshal_acks")
            return
        n, na = width * self.op, width * self.ack_size   # this rank's own row: all empty slots
        check(_L.hkv_wl_marshal_acks_aligned(_ptr(self.inv_recv[self.rank * n:]), _ptr(self.inv_totals[self.rank:]), 1,
                                             width, self.op, _ptr(self.ack_slab[self.rank * na:]), self.ack_size,
                                             self.rank, _s()), "marshal_acks")

    def _inv_launch(self, p: int, width: int):
        """peer p's row of inv_recv as one unique-key launch; with fused_acks it also writes the ACKs
        answering them into ack_slab's row p, lined up with the INVs (positions past the row's total
        are never read: the peer's ACK launch stops at its own total)"""
        n = width * self.op
        if self.fused_acks:
            self.kvs.batch(L.BatchType.invs, self.inv_recv[p * n:], 1, width, self.op, self.mb,
                           counts=self.inv_totals[p:p + 1], unique=True,
                           ack_out=self.ack_slab[p * width * self.ack_size:], ack_out_size=self.ack_size)
        else:
            self.kvs.batch(L.BatchType.invs, self.inv_recv[p * n:], 1, width, self.op, self.mb,
                           counts=self.inv_totals[p:p + 1], unique=True)

    # -- per-peer exchanges (ReplicaGroupRound with p2p): each peer's INV slab is sent and received on
    # its own, applied as soon as it is there, and its ACK row goes back right after
    def inv_row_io(self, p: int, width: int):
        """(send, receive) of the INV exchange with peer p: this rank's packed slab, p's row"""
        n = width * self.op
        return self.inv_pack[:n], self.inv_recv[p * n:(p + 1) * n]

    def ack_row_io(self, p: int, width: int):
        """(send, receive) of the ACK exchange with peer p: the answers to p's INVs, p's answers to ours"""
        n = width * self.ack_size
        return self.ack_slab[p * n:(p + 1) * n], self.ack_recv[p * n:(p + 1) * n]

    def invs_begin(self, width: int):
        """Before the per-peer INV launches: this rank's own row carries nothing, and the ACK row it
        'receives' from itself is all empty slots (the ACK phase reads every row)"""
        self.inv_totals[self.rank:self.rank + 1].zero_()
        n, na = width * self.op, width * self.ack_size
        check(_L.hkv_wl_marshal_acks_aligned(_ptr(self.inv_recv[self.rank * n:]), _ptr(self.inv_totals[self.rank:]), 1,
                                             width, self.op, _ptr(self.ack_recv[self.rank * na:]), self.ack_size,
                                             self.rank, _s()), "marshal_acks")
        if self.failed:   # no ACKs from a failed replica
            self.ack_slab[:self.N * na].view(-1, self.ack_size)[:, 8] = int(L.Bucket.EMPTY)

    def invs_peer(self, p: int, width: int, fold: bool):
        """Peer p's INVs (its row of inv_recv, just arrived) as one unique-key launch, then the ACK row
        answering them. fold: p's total rides in the row's spare slot (steady rounds)"""
        n = width * self.op
        if fold:
            a = p * n + (width - 1) * self.op
            self.inv_totals[p:p + 1].copy_(self.inv_recv[a:a + 4].view(torch.int32))
        if self.failed:
            return
        self._inv_launch(p, width)
        if not self.fused_acks:
            check(_L.hkv_wl_marshal_acks_aligned(_ptr(self.inv_recv[p * n:]), _ptr(self.inv_totals[p:]), 1, width,
                                                 self.op, _ptr(self.ack_slab[p * width * self.ack_size:]), self.ack_size,
                                                 self.rank, _s()), "marshal_acks")

    def invs_end(self, width: int):
        if self.count_elems and not self.failed:
            self.elem_totals[0] += self.inv_totals.sum()

    def acks(self, width: int, stride: int):
        """Apply the ACKs returned by the peers (ack_recv [N][width], row p from rank p, lined up
        with inv_pack), regrouped per worker ([W][stride]); the VALs of completed writes, packed
        (val_pack)."""
        N, W, C = self.N, self.W, self.C
        if self.failed:
            self.val_off[W:].zero_()
            return
        if self.unique_acks:
            # row p of ack_recv: peer p's ACKs lined up with inv_pack, worker w's at [inv_off[w], inv_off[w+1]);
            # without the total read back, the launch spans the width and ends at inv_off[W]
            T = self.own_total if self.own_total is not None else width
            if T and self.ack_rows:
                self.kvs.batch(L.BatchType.acks, self.ack_recv, W, T, self.ack_size, self.mb, rw=self.ops,
                               rw_stride_bytes=LOCAL * self.op, offsets=self.inv_off, rw_state=self.states,
                               unique=True, rows=(N, width, self.rank), rw_opcodes=self._rwo())
            elif T:
                for p in range(N):
                    if p != self.rank:
                        self.kvs.batch(L.BatchType.acks, self.ack_recv[p * width * self.ack_size:], W, T, self.ack_size,
                                       self.mb, rw=self.ops, rw_stride_bytes=LOCAL * self.op, offsets=self.inv_off,
                                       rw_state=self.states, unique=True, rw_opcodes=self._rwo())
            if self.count_elems:
                self.elem_totals[1] += (N - 1) * self.inv_off[W]
            check(_L.hkv_wl_collect_vals_rows(_ptr(self.ack_recv), W, N, width, self.ack_size, _ptr(self.val_slab), C,
                                              _ptr(self.val_count), self.rank, _ptr(self.held[1:]), _ptr(self.inv_off),
                                              _s()), "collect_vals_rows")
            check(_L.hkv_wl_pack_rows(_ptr(self.val_slab), _ptr(self.val_count), W, C, L.OP_META_SIZE,
                                      _ptr(self.val_pack), _ptr(self.val_off), _s()), "pack vals")
            return
        check(_L.hkv_wl_regroup_aligned(_ptr(self.ack_recv), N, width, _ptr(self.inv_off), _ptr(self.inv_count), W,
                                        self.ack_size, _ptr(self.ack_batch), stride, _ptr(self.ack_batch_count),
                                        _s()), "regroup")
        if self.count_elems:
            self.elem_totals[1] += self.ack_batch_count.sum()
        self.kvs.batch(L.BatchType.acks, self.ack_batch, W, stride, self.ack_size, self.mb,
                       counts=self.ack_batch_count, rw=self.ops, rw_stride_bytes=LOCAL * self.op, rw_state=self.states,
                       rw_opcodes=self._rwo())
        check(_L.hkv_wl_collect_vals(_ptr(self.ack_batch), _ptr(self.ack_batch_count), W, stride, self.ack_size,
                                     _ptr(self.val_slab), C, _ptr(self.val_count), self.rank,
                                     _ptr(self.held[1:]), None, _s()), "collect_vals")
        check(_L.hkv_wl_pack_rows(_ptr(self.val_slab), _ptr(self.val_count), W, C, L.OP_META_SIZE,
                                  _ptr(self.val_pack), _ptr(self.val_off), _s()), "pack vals")

    def _rwo(self):
        """the opcode mirror the ACK launches complete from"""
        return self.opcodes

    def vals(self, width: int):
        """Apply the gathered VALs of the peers ([N][width], row p: val_totals[p] VALs)."""
        if self.failed:
            return
        self.val_totals[self.rank:self.rank + 1].zero_()
        if self.count_elems:
            self.elem_totals[2] += self.val_totals.sum()
        self.kvs.batch(L.BatchType.vals, self.val_recv, self.N, width, L.OP_META_SIZE, self.mb,
                       counts=self.val_totals)

    def membership_change(self, peer: int | None = None, membership: bytes | None = None):
        """The group drops `peer` (group_membership_update, inline-util.h:26-43), or takes the
        spacetime_group_membership Hades agreed on (`membership`). Every worker runs the
        after-membership-change batch over its ops (hermes_worker.c:526-542); the VALs of the
        writes and replays it completed are packed into val_pack for one more VAL exchange
        (memb_change_* callbacks, hermes_worker.c:163-203). A failed replica, or one whose
        membership did not change (both None), sends none."""
        W, C = self.W, self.C
        if self.failed or (peer is None and membership is None):
            self.val_off[W:].zero_()
            return
        if membership is not None:
            g = membership[1]
            if bin(g).count("1") < self.N // 2:   # inline-util.h:39-42: "Majority is down!"
                raise MajorityLost(f"replica {self.rank}: membership {g:#04x} of {self.N}")
            self.mb = bytes(membership[:3]) + bytes(5)
        else:
            g = self.mb[1] & ~(1 << peer) & 0xFF
            self.mb = L.membership(0, self.rank, alive=g)
        self.kvs.batch(L.BatchType.local_ops_after_membership_change, self.ops, W, LOCAL, self.op, self.mb,
                       state_out=self.states)
        check(_L.hkv_wl_marshal_memb_vals(_ptr(self.ops), W, LOCAL, self.op, _ptr(self.val_slab), C,
                                          _ptr(self.val_count), self.rank, _ptr(self.states), _s()), "marshal_memb_vals")
        check(_L.hkv_wl_pack_rows(_ptr(self.val_slab), _ptr(self.val_count), W, C, L.OP_META_SIZE,
                                  _ptr(self.val_pack), _ptr(self.val_off), _s()), "pack memb vals")

    def val_width(self) -> int:
        """After the VAL totals are gathered (host synchronisation): the largest of them"""
        return max(1, int(self.val_totals.max().item()))

    def fold_counters(self) -> torch.Tensor:
        """counters[0..4] brought up to date (refill leaves per-worker-group partial sums)"""
        check(_L.hkv_wl_fold_counters(_ptr(self.counters), _s()), "fold_counters")
        return self.counters

    def stats(self) -> dict:
        c = self.fold_counters()[:3].cpu().tolist()
        h = self.held.cpu().tolist()
        return {"committed": c[0], "misses": c[1], "writes_completed": c[2], "invs_held": h[0], "vals_dropped": h[1]}


class WidthPlan:
    """The slab width of a replica group's rounds without a host read per round. Every
    `calib_every`-th round (and the first) reads the round's largest INV total back, as before; the
    rounds in between use width = slack x that total + pad and cap each rank's INVs at it (the rest
    are held in PUT_SUCCESS, like credit-held INVs, and go out later). Every rank reads the same
    all-gathered totals, so every rank picks the same width. A round with a failure, Hades or the
    regrouped ACK path always reads back."""

    def __init__(self):
        self.calib_every = int(os.environ.get("HKV_GROUP_CALIB", "16"))
        self.slack = float(os.environ.get("HKV_GROUP_WIDTH_SLACK", "1.25"))
        self.pad = 256
        # the totals ride in one spare slot of each slab (HKV_GROUP_FOLD_TOTALS=0: their own all-gathers)
        self.fold = os.environ.get("HKV_GROUP_FOLD_TOTALS", "1") != "0"
        self.width = None
        self.k = 0

    def steady(self, special: bool) -> bool:
        """whether this round runs at the planned width (call once per round)"""
        k, self.k = self.k, self.k + 1
        return (self.calib_every > 0 and self.width is not None and not special and k % self.calib_every != 0)

    def calibrate(self, width: int, cap: int) -> None:
        """cap: the slab capacity in slots (one is kept for the spare slot)"""
        self.width = min(cap - 1, int(width * self.slack) + self.pad)

    def slab_width(self) -> int:
        """slots per slab in a steady round: the INV cap, plus the spare slot when the totals ride in it"""
        return self.width + 1 if self.fold else self.width


class _HostStaged:
    """a gloo exchange staged through host buffers: wait() ends the exchange and copies the received row
    to the device tensor (on the current stream)"""

    def __init__(self, works, host_rcv, rcv, host_snd):
        self.works, self.host_rcv, self.rcv, self.host_snd = works, host_rcv, rcv, host_snd

    def wait(self):
        for w in self.works:
            w.wait()
        self.rcv.copy_(self.host_rcv)


def _timed(events, name, fn, only=None):
    if events is None or (only is not None and name not in only):
        fn()
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    events.setdefault(name, []).append((a, b))


class ReplicaGroupRound:
    """One replica per process; the exchanges are RCCL collectives (torch.distributed "nccl",
    or any backend whose all_gather_into_tensor / all_to_all_single take these tensors)."""

    LOCAL = LOCAL

    def __init__(self, kvs: HermesKV | None, n_workers: int, zipf: HkvZipf | None, write_permille: int = 200, *,
                 seed: int = 0x5EED, world: int, rank: int, group=None, replica=None, hades: bool = False,
                 comm=None, p2p: bool | None = None, **kw):
        """`replica`: drive an existing ReplicaRound-shaped object instead of building one.
        `hades`: the membership comes from Hades agreement over heartbeats exchanged every round
        (a failed rank is expelled when the survivors agree), instead of a host-driven drop.
        `comm`: an object with gather(out, inp), gather_async(out, inp) -> work (.wait()), a2a(out, inp)
        and p2p(pairs) -> {peer: [work]} to use instead of torch.distributed (tests: ranks as threads of
        one process). `p2p` (default: HKV_GROUP_P2P, on): the INV slabs and ACK rows go peer by peer
        (grouped isend/irecv per peer) instead of one all-gather and one all-to-all, so each peer's INV
        launch waits only for that peer's slab and its ACK row leaves right after it."""
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.comm = comm
        self.p2p = (os.environ.get("HKV_GROUP_P2P", "1") != "0") if p2p is None else p2p
        self.r = replica if replica is not None else ReplicaRound(kvs, n_workers, world, rank, zipf,
                                                                  write_permille, seed=seed, **kw)
        self.hades = hades
        self.world = world
        if hades:
            self.r.hades_start()
            self._hades_bootstrap()
        self.R = world - 1
        self.rstride = self.r.C * self.R
        self.counters = self.r.counters
        self.fold_counters = self.r.fold_counters
        self.plan = WidthPlan() if getattr(self.r, "packed_marshal", False) else None
        self.inv_total = self.r.inv_total
        self.elem_totals = self.r.elem_totals

    @property
    def count_elems(self) -> bool:
        return self.r.count_elems

    @count_elems.setter
    def count_elems(self, v: bool) -> None:
        self.r.count_elems = v

    def _gather(self, out, inp):
        if self.comm is not None:
            return self.comm.gather(out, inp)
        self.dist.all_gather_into_tensor(out, inp, group=self.group)

    def _gather_async(self, out, inp):
        """the same all-gather, returned unwaited: the collective runs on the backend's stream (RCCL's
        own) while torch's stream goes on; work.wait() orders the consumer after it"""
        if self.comm is not None:
            return self.comm.gather_async(out, inp)
        return self.dist.all_gather_into_tensor(out, inp, group=self.group, async_op=True)

    def _a2a(self, out, inp):
        if self.comm is not None:
            return self.comm.a2a(out, inp)
        self.dist.all_to_all_single(out, inp, group=self.group)

    def _p2p(self, pairs) -> dict:
        """pairs: (peer, send, receive), peers ascending. One grouped isend/irecv per peer, returned
        unwaited: {peer: [work]}. Every rank walks its peers in ascending order, which is one global
        order of the rank pairs, so the exchanges cannot wait on each other in a cycle."""
        if self.comm is not None:
            return self.comm.p2p(pairs)
        d = self.dist
        if pairs and pairs[0][1].is_cuda and d.get_backend(self.group) != "nccl":
            # gloo (tests: ranks sharing one GPU): its point-to-point ops move host memory and are not
            # ordered on the CUDA stream, so the rows are staged through host buffers
            out = {}
            for p, snd, rcv in pairs:
                sc, rc = snd.cpu(), torch.empty(rcv.shape, dtype=rcv.dtype)
                ws = d.batch_isend_irecv([d.P2POp(d.isend, sc, p, self.group), d.P2POp(d.irecv, rc, p, self.group)])
                out[p] = [_HostStaged(ws, rc, rcv, sc)]
            return out
        return {p: d.batch_isend_irecv([d.P2POp(d.isend, snd, p, self.group), d.P2POp(d.irecv, rcv, p, self.group)])
                for p, snd, rcv in pairs}

    def _views(self, changed: bool) -> bytes:
        """one heartbeat exchange: all ranks' rows gathered (row = sender), this rank polls its
        column. Returns the gathered table."""
        r, n = self.r, self.world
        row = torch.tensor(list(r.hades_row(changed)), dtype=torch.uint8, device=r.ops.device)
        out = torch.empty(n * row.numel(), dtype=torch.uint8, device=r.ops.device)
        self._gather(out, row)
        table = bytes(out.cpu().tolist())
        if not r.failed:
            w = 4 * n + 4
            r.hades.receive_column(b"".join(table[s * w:s * w + 4 * n] for s in range(n)))
        return table

    def _trailers(self, table: bytes) -> list[bytes]:
        w = 4 * self.world + 4
        return [table[s * w + 4 * self.world:(s + 1) * w] for s in range(self.world)]

    def _hades_bootstrap(self, max_periods: int = 16):
        """spin_until_all_nodes_are_in_membership (hermes_worker.c:245-259): heartbeat periods
        until every rank's membership is the whole group"""
        for _ in range(max_periods):
            self.r.hades.update()
            if all(t[1] for t in self._trailers(self._views(False))):
                return
        raise RuntimeError("Hades bootstrap did not reach the full membership")

    def _hades_period(self):
        """update_view_and_issue_hbs + group_membership_update + poll_for_remote_views
        (hermes_worker.c:262-291); when any rank's membership changed, the ranks whose membership
        changed run the after-membership-change batch and every rank joins one VAL exchange"""
        r = self.r
        changed, mb = False, None
        if not r.failed:
            changed, mb, _ = r.hades.update()
        table = self._views(changed)
        if any(t[0] for t in self._trailers(table)):
            r.membership_change(membership=mb if changed else None)
            self._gather(*r.val_total_io())
            w2 = r.val_width()
            self._gather(*r.val_io(w2))
            r.vals(w2)

    def step(self, events: dict | None = None, timed_batches=None, drop: int | None = None):
        """One protocol round. `drop`: that rank fails once its INVs of this round are out (no
        ACKs or VALs from it); the round ends with a membership change and one more VAL
        exchange for the writes it completes -- or, with Hades, the failed rank stops
        heartbeating and the survivors expel it when they agree (two periods later)."""
        r = self.r
        p2p = self.p2p and hasattr(r, "invs_peer")
        steady = self.plan is not None and self.plan.steady(drop is not None or self.hades or not r.unique_acks)
        fold = steady and self.plan.fold
        if steady:   # no host read: the planned width, each rank's INVs capped at it
            width, stride = self.plan.slab_width(), None
            r.own_total = None
            _timed(events, "local", lambda: r.local(cap=self.plan.width), timed_batches)
            if fold and p2p:
                r.inv_io_total(width)          # the total into the slab's spare slot; the rows go peer by peer
            elif fold:
                self._gather(*r.inv_io_total(width))
                r.take_inv_totals(width)
            else:
                self._gather(*r.inv_total_io())
        else:
            _timed(events, "local", r.local, timed_batches)
            self._gather(*r.inv_total_io())
            width, stride = r.round_shape()  # host synchronisation: this round's exact width
            if self.plan is not None:
                self.plan.calibrate(width, r.W * r.C)
        if p2p:
            peers = [p for p in range(self.world) if p != r.rank]
            inv_w = self._p2p([(p, *r.inv_row_io(p, width)) for p in peers])
        elif not fold:
            self._gather(*r.inv_io(width))
        if drop is not None:
            r.peer_failing()
            if drop == r.rank:
                r.fail()
        if p2p:
            ack_w = {}

            def invs():
                r.invs_begin(width)
                for p in peers:   # each peer's launch waits for that peer's slab only
                    for w in inv_w[p]:
                        w.wait()
                    r.invs_peer(p, width, fold)
                    ack_w.update(self._p2p([(p, *r.ack_row_io(p, width))]))
                r.invs_end(width)
            _timed(events, "invs", invs, timed_batches)
            for p in peers:
                for w in ack_w[p]:
                    w.wait()
        else:
            _timed(events, "invs", lambda: r.invs(width), timed_batches)
            self._a2a(*r.ack_io(width))
        _timed(events, "acks", lambda: r.acks(width, stride), timed_batches)
        if not self.hades and drop is None:
            # the VAL exchange overlaps the refill: the refill touches only this replica's op slab and
            # its mirrors, the VAL batch only the table, so their order does not matter
            if fold:
                w_val = self._gather_async(*r.val_io_total(width))
                r.refill()
                w_val.wait()
                r.take_val_totals(width)
            else:
                w_tot = self._gather_async(*r.val_total_io())
                w_val = self._gather_async(*r.val_io(width))
                r.refill()
                w_tot.wait()
                w_val.wait()
            _timed(events, "vals", lambda: r.vals(width), timed_batches)
            return
        self._gather(*r.val_total_io())
        self._gather(*r.val_io(width))
        _timed(events, "vals", lambda: r.vals(width), timed_batches)
        if self.hades:
            self._hades_period()
        elif drop is not None:
            r.membership_change(drop)
            self._gather(*r.val_total_io())
            w2 = r.val_width()
            self._gather(*r.val_io(w2))
            r.vals(w2)
        r.refill()

    def stats(self) -> dict:
        return self.r.stats()


def census_row(census) -> torch.Tensor:
    """What a replica contributes to a group census, on the device: (digest_sum, digest_xor, keys, keys that
    are not VALID) as int64 (the unsigned words' bit patterns), made from HermesKV.census() without a host
    read."""
    from .kvs import CENSUS_FIELDS
    t = census.tensor
    w = {n: CENSUS_FIELDS[n][0] for n in ("digest_sum", "digest_xor", "keys", "by_state")}
    keys = t[w["keys"]]
    return torch.stack([t[w["digest_sum"]], t[w["digest_xor"]], keys, keys - t[w["by_state"] + int(L.State.VALID)]])


def census_rows_agree(rows: list, live_ranks) -> bool:
    """whether every live rank's (digest_sum, digest_xor, keys) is the same"""
    live = [tuple(rows[r][:3]) for r in live_ranks]
    return all(x == live[0] for x in live)


def group_census(kvs: HermesKV, group=None, live_ranks=None) -> dict:
    """Whether the live replicas of a group hold the same table: every rank takes the census of its own table
    (HermesKV.census: in place, from whichever residency the table is in) and one all_gather_into_tensor moves
    census_row() of every rank, on torch's current stream and with no host read before it (gloo takes the CUDA
    tensors as NCCL / RCCL does). Collective: every rank of `group` calls it, a failed one too (its row is
    gathered and left out of the comparison by live_ranks, default: all ranks). Returns the same on every rank:
    rows[r] = [digest_sum, digest_xor, keys, not VALID] of rank r as unsigned integers, live_ranks,
    live_ranks_agree (digest and key count equal on all live ranks) and not_valid (rows' last column)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    row = census_row(kvs.census())
    out = torch.empty(world * row.numel(), dtype=torch.int64, device=row.device)
    dist.all_gather_into_tensor(out, row, group=group)
    rows = [[int(x) & 0xFFFFFFFFFFFFFFFF for x in r] for r in out.view(world, -1).cpu().tolist()]
    live = list(range(world)) if live_ranks is None else [int(r) for r in live_ranks]
    return {"rows": rows, "live_ranks": live, "live_ranks_agree": census_rows_agree(rows, live),
            "not_valid": [r[3] for r in rows]}


class _RecordSink:
    """Where a repair's records go: HermesKV.install (insert False: today's path and today's dict), or
    HermesKV.upsert, which also inserts the keys the table lacks. result(): the summed counts {raised, equal, older,
    missed}; with insert, missed is 0 and inserted, replaced and evictions are added."""

    def __init__(self, kvs: HermesKV, insert: bool, dev):
        self.kvs, self.insert = kvs, bool(insert)
        self.tot = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ups = dict.fromkeys(("raised", "equal", "older", "inserted", "replaced", "evictions"), 0)

    def __call__(self, records, n: int) -> None:
        if not self.insert:
            self.tot += self.kvs.install(records, n=n).tensor
            return
        r = self.kvs.upsert(records, n=n)
        for k in self.ups:
            self.ups[k] += r[k]

    def result(self) -> dict:
        if not self.insert:
            return {k: int(v) for k, v in zip(("raised", "equal", "older", "missed"), self.tot.cpu().tolist())}
        u = self.ups
        return {"raised": u["raised"], "equal": u["equal"], "older": u["older"], "missed": 0,
                "inserted": u["inserted"], "replaced": u["replaced"], "evictions": u["evictions"]}


def _bucket_chunks(num_bkts: int, chunk_buckets: int | None):
    step = int(chunk_buckets) if chunk_buckets else int(num_bkts)
    assert step > 0
    return [(lo, min(lo + step, int(num_bkts))) for lo in range(0, int(num_bkts), step)]


def resync(dst: HermesKV, src: HermesKV, chunk_buckets: int | None = None, min_ts: int = 0,
           insert: bool = False) -> dict:
    """Repair a stale replica from a live one, both tables in this process (loopback groups, one-GPU tests): walk
    `src` in chunks of chunk_buckets buckets (default: the whole table at once), HermesKV.extract each chunk into
    one reused buffer and HermesKV.install it into `dst`, which may have another bucket count, log order or
    residency. Returns the summed install counts {raised, equal, older, missed} plus records and scanned_keys.
    Each chunk's record count is read on the host (the buffer is sized once, for the fullest chunk possible:
    eight keys per bucket, at most the source's keys). After a resync of a quiet group the two tables' census
    digests are equal. Sound only while `dst` takes no client operations; INVs it receives meanwhile are safe,
    the install being timestamp-guarded (an older record changes nothing). min_ts only saves volume -- there is
    no global watermark in a per-key protocol. Membership re-admission is not done here.
    insert=True: each chunk goes through HermesKV.upsert instead, which inserts the keys `dst` lacks as the
    reference inserts (include/hermeskv.h, "Upsert"); `missed` is then 0 and inserted, replaced and evictions are
    added to the dict. `dst` may then be empty (created with populate=False): a rebuild. What can still leave the
    tables' digests apart: `dst` is newer in a key (`older`), or keys were lost to the lossy index -- an insert
    that `replaced` a live slot of the same tag, or an eviction; both are counted, never hidden."""
    assert dst.sizes == src.sizes, "records of one entry size only"
    chunks = _bucket_chunks(src.cfg.num_bkts, chunk_buckets)
    cap = max(1, min(int(src.num_keys), 8 * max(hi - lo for lo, hi in chunks)))
    dev = torch.device("cuda", src.device)
    buf = torch.empty(cap * src.sizes.entry, dtype=torch.uint8, device=dev)
    res = torch.empty(2, dtype=torch.int64, device=dev)
    sink = _RecordSink(dst, insert, dev)
    records = scanned = 0
    for lo, hi in chunks:
        x = src.extract((lo, hi), min_ts, out=buf, result=res)
        h = x.host()
        assert h["records"] <= cap, "more live keys in a chunk than slots"
        records, scanned = records + h["records"], scanned + h["scanned_keys"]
        if h["records"]:
            sink(x, h["records"])
    out = sink.result()
    out.update(records=records, scanned_keys=scanned)
    return out


def group_resync(kvs: HermesKV, group, source_rank: int, stale_ranks, chunk_buckets: int | None, min_ts: int = 0,
                 insert: bool = False) -> dict:
    """resync() across ranks. Collective: every rank of `group` calls it with the same arguments and its own table
    (tables of one entry size; bucket counts may differ -- the chunks walk the source's, whose count is broadcast
    first). Per chunk the source rank extracts and broadcasts the record count, then the records (CUDA tensors
    through torch.distributed: gloo and NCCL / RCCL alike); only the ranks in stale_ranks install, the others
    just take part in the broadcasts. Returns this rank's summed install counts (zeros where it did not install)
    plus records and scanned_keys of the source. The same conditions as resync(): a stale rank takes no client
    operations meanwhile, and nobody is re-admitted to the membership here. insert=True: the stale ranks upsert
    (resync()'s insert: inserted, replaced and evictions in the dict, missed 0; a stale rank may be empty)."""
    import torch.distributed as dist
    rank = dist.get_rank(group)
    src = dist.get_global_rank(group, source_rank) if group is not None else int(source_rank)
    stale = {int(r) for r in stale_ranks}
    assert source_rank not in stale
    dev = torch.device("cuda", kvs.device)
    E = kvs.sizes.entry
    geo = torch.tensor([kvs.cfg.num_bkts, kvs.num_keys], dtype=torch.int64, device=dev)
    dist.broadcast(geo, src, group=group)
    num_bkts, src_keys = (int(v) for v in geo.cpu().tolist())
    chunks = _bucket_chunks(num_bkts, chunk_buckets)
    cap = max(1, min(src_keys, 8 * max(hi - lo for lo, hi in chunks)))
    buf = torch.empty(cap * E, dtype=torch.uint8, device=dev)
    res = torch.zeros(2, dtype=torch.int64, device=dev)
    sink = _RecordSink(kvs, insert, dev)
    records = scanned = 0
    for lo, hi in chunks:
        if rank == source_rank:
            kvs.extract((lo, hi), min_ts, out=buf, result=res)
        dist.broadcast(res, src, group=group)
        n, sc = (int(v) for v in res.cpu().tolist())
        assert n <= cap, "more live keys in a chunk than slots"
        records, scanned = records + n, scanned + sc
        if not n:
            continue
        dist.broadcast(buf[:n * E], src, group=group)
        if rank in stale:
            sink(buf, n)
    out = sink.result()
    out.update(records=records, scanned_keys=scanned)
    return out


def part_diff(rows_a, rows_b, mask: torch.Tensor | None = None):
    """hkv_part_rows_diff_async on two partition censuses of the same part_bits (PartRows of
    HermesKV.census_parts, or their [P, 4] int64 tensors): (mask, count), both on the device and with no host
    read -- mask uint8[P], 1 where the two rows differ in any word; count int64[1], the non-zero bytes of mask.
    Given `mask` (uint8[P], written in place), the result is or-ed into it: the union over several peers."""
    a = getattr(rows_a, "tensor", rows_a)
    b = getattr(rows_b, "tensor", rows_b)
    assert a.shape == b.shape and a.dim() == 2 and a.shape[1] == 4, "two [P, 4] row tensors of one part_bits"
    assert all(t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() for t in (a, b)) and a.device == b.device
    P = a.shape[0]
    part_bits = P.bit_length() - 1
    assert P == 1 << part_bits
    accumulate = mask is not None
    if mask is None:
        mask = torch.empty(P, dtype=torch.uint8, device=a.device)
    assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == P
    count = torch.empty(1, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        s = torch.cuda.current_stream(a.device).cuda_stream
        check(raw().hkv_part_rows_diff_async(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), part_bits,
                                             ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                             int(accumulate), ctypes.c_void_p(s)), "hkv_part_rows_diff_async")
    return mask, count


def _selected_keys(rows_src: torch.Tensor, mask: torch.Tensor, count: torch.Tensor):
    """(the source's live keys in the selected partitions -- the masked extract's record count, exact --, count)
    in one host read"""
    n = (rows_src[:, 2] * (mask != 0)).sum()
    return tuple(int(v) for v in torch.stack([n, count[0]]).cpu().tolist())


def _delta_verify(kvs: HermesKV, rows_src: torch.Tensor, part_bits: int) -> dict:
    """the target's partition census again, against the source's rows: what still differs is reported"""
    mask, count = part_diff(rows_src, kvs.census_parts(part_bits))
    n = int(count.cpu()[0])
    left = torch.nonzero(mask)[:64, 0].cpu().tolist() if n else []
    return {"differing_after": n, "unresolved": [int(p) for p in left]}


def _log2_buckets(num_bkts: int) -> int:
    return int(num_bkts).bit_length() - 1


def delta_resync(dst: HermesKV, src: HermesKV, part_bits: int | None = None, chunk_buckets: int | None = None,
                 insert: bool = False) -> dict:
    """resync() that ships only the partitions that differ (include/hermeskv.h, "Partitioned census and delta
    repair"), both tables in this process. In this order: HermesKV.census_parts of both tables at part_bits
    (default: min(20, log2 of the smaller bucket count); at most log2 of either bucket count, so that every key of a
    bucket lies in one partition whatever the geometry); part_diff; one host read of the source's key count in the
    differing partitions, which sizes the record buffer exactly; the masked extract of `src` (in chunks of
    chunk_buckets buckets, default the whole table, each chunk's count read on the host) and the install into `dst`;
    the partition census of `dst` again, diffed against the source's rows.
    Returns the summed install counts {raised, equal, older, missed} plus records and scanned_keys (of the selected
    buckets only), partitions (2^part_bits), differing_before, differing_after and unresolved: the partitions that
    still differ, at most 64 listed. A partition that still differs is reported, never hidden; two causes are
    known: the target is newer in a key (its record counts as `older`), or the target lacks the key or shadows it
    (its record counts as `missed`). Equal keys of a differing partition are shipped too and count as `equal`: the
    install is timestamp-guarded. Every limit of resync() holds: sound only while `dst` takes no client operations
    (INVs it receives meanwhile are safe); nothing is inserted; nobody is re-admitted to the membership; extract and
    install refuse tables with RMWs.
    insert=True: the records go through HermesKV.upsert, which inserts the keys `dst` lacks (include/hermeskv.h,
    "Upsert"); `missed` is 0 and inserted, replaced and evictions are added. A partition can then still be in
    unresolved for two reasons: `dst` is newer in a key (`older`), or keys were lost to `replaced` / `evictions`
    (the reference's lossy index: an insert took a live slot). Such partitions are reported, never hidden."""
    assert dst.sizes == src.sizes, "records of one entry size only"
    if part_bits is None:
        part_bits = min(20, _log2_buckets(min(src.cfg.num_bkts, dst.cfg.num_bkts)))
    part_bits = int(part_bits)
    dev = torch.device("cuda", src.device)
    rows = src.census_parts(part_bits).tensor
    mask, count = part_diff(rows, dst.census_parts(part_bits))
    n, differing = _selected_keys(rows, mask, count)
    sink = _RecordSink(dst, insert, dev)
    records = scanned = 0
    if n:
        buf = torch.empty(n * src.sizes.entry, dtype=torch.uint8, device=dev)
        res = torch.empty(2, dtype=torch.int64, device=dev)
        for lo, hi in _bucket_chunks(src.cfg.num_bkts, chunk_buckets):
            x = src.extract((lo, hi), out=buf, result=res, part_bits=part_bits, part_mask=mask)
            h = x.host()
            records, scanned = records + h["records"], scanned + h["scanned_keys"]
            if h["records"]:
                sink(x, h["records"])
        assert records == n, "the selected partitions' key counts are the masked extract's records"
    out = sink.result()
    out.update(records=records, scanned_keys=scanned, partitions=1 << part_bits, differing_before=differing)
    out.update(_delta_verify(dst, rows, part_bits))
    return out


def group_delta_resync(kvs: HermesKV, group, source_rank: int, stale_ranks, part_bits: int | None,
                       chunk_buckets: int | None, insert: bool = False) -> dict:
    """delta_resync() across ranks. Collective: every rank of `group` calls it with the same arguments and its own
    table (tables of one entry size; bucket counts may differ). part_bits None: min(20, log2 of the smallest bucket
    count of the group), agreed by an all_reduce. The source rank broadcasts its partition rows; each stale rank
    diffs them against its own; the masks are united over the ranks (all_reduce MAX of uint8, which gloo and NCCL /
    RCCL both take); every rank reads the source's key count in the union -- the exact record count -- from the
    rows it now holds. Per chunk the source extracts with the union mask and broadcasts the count, then the
    records; only the ranks in stale_ranks install, and they alone take their partition census again and diff it
    against the source's rows. Returns this rank's install counts (zeros where it did not install), records and
    scanned_keys of the source, partitions, selected (partitions in the union), and this rank's differing_before,
    differing_after and unresolved (0, 0 and [] where it is not stale). A stale rank's `equal` therefore covers
    the keys of the partitions only another stale rank differed in. The conditions are delta_resync()'s: a stale
    rank takes no client operations meanwhile, nothing is inserted, nobody is re-admitted to the membership here,
    no tables with RMWs; a partition that still differs (the rank is newer in a key: `older`; it lacks or shadows
    a key: `missed`) is reported in unresolved. insert=True: the stale ranks upsert (delta_resync()'s insert:
    inserted, replaced and evictions in the dict, missed 0); a partition still in unresolved is then one where the
    rank is newer in a key or lost keys to `replaced` / `evictions`."""
    import torch.distributed as dist
    rank = dist.get_rank(group)
    src = dist.get_global_rank(group, source_rank) if group is not None else int(source_rank)
    stale = {int(r) for r in stale_ranks}
    assert source_rank not in stale
    dev = torch.device("cuda", kvs.device)
    E = kvs.sizes.entry
    geo = torch.tensor([kvs.cfg.num_bkts, _log2_buckets(kvs.cfg.num_bkts)], dtype=torch.int64, device=dev)
    low = geo[1:].clone()
    dist.broadcast(geo, src, group=group)
    dist.all_reduce(low, op=dist.ReduceOp.MIN, group=group)
    num_bkts, most_bits = int(geo[0].cpu()), int(low.cpu()[0])
    part_bits = min(20, most_bits) if part_bits is None else int(part_bits)
    assert part_bits <= most_bits, "part_bits above log2 of a rank's bucket count"
    P = 1 << part_bits
    mine = kvs.census_parts(part_bits).tensor
    rows = mine.clone()
    dist.broadcast(rows, src, group=group)
    mask = torch.zeros(P, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    if rank in stale:
        mask, count = part_diff(rows, mine)
    differing = count.clone()
    dist.all_reduce(mask, op=dist.ReduceOp.MAX, group=group)
    n, selected = _selected_keys(rows, mask, (mask != 0).sum().reshape(1))
    sink = _RecordSink(kvs, insert, dev)
    records = scanned = 0
    if n:
        buf = torch.empty(n * E, dtype=torch.uint8, device=dev)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        for lo, hi in _bucket_chunks(num_bkts, chunk_buckets):
            if rank == source_rank:
                kvs.extract((lo, hi), out=buf, result=res, part_bits=part_bits, part_mask=mask)
            dist.broadcast(res, src, group=group)
            m, sc = (int(v) for v in res.cpu().tolist())
            assert records + m <= n, "more records than the selected partitions' keys"
            records, scanned = records + m, scanned + sc
            if not m:
                continue
            dist.broadcast(buf[:m * E], src, group=group)
            if rank in stale:
                sink(buf, m)
    out = sink.result()
    out.update(records=records, scanned_keys=scanned, partitions=P, selected=selected,
               differing_before=int(differing.cpu()[0]))
    out.update(_delta_verify(kvs, rows, part_bits) if rank in stale else {"differing_after": 0, "unresolved": []})
    return out


NEED_CLASSES = ("missed", "newer", "validate", "same", "state_only", "older")   # hkv_need_result's first six words


def _key_delta_bytes(E: int, summaries: int, needed: int) -> dict:
    """what a key-level repair ships, beside what the partitioned delta would have shipped for the same partitions"""
    return {"bytes_summaries": 16 * summaries, "bytes_keys": 8 * needed, "bytes_records": E * needed,
            "bytes_partition_delta": E * summaries}


def key_delta_resync(dst: HermesKV, src: HermesKV, part_bits: int | None = None, chunk_buckets: int | None = None,
                     insert: bool = False) -> dict:
    """delta_resync() that ships key summaries first and then only the records `dst` needs (include/hermeskv.h,
    "Key-level delta repair"), both tables in this process. In this order: both partition censuses and part_diff,
    as delta_resync(); one host read of the source's key count in the differing partitions -- the exact summary
    count; HermesKV.summaries of `src` for those partitions (16 bytes per key); HermesKV.need of `dst` (the keys
    whose install would miss or change a digest byte: missed, newer, validate); one host read of `needed`;
    HermesKV.fetch of those keys from `src` (every one must be found there); install into `dst` (insert=True:
    upsert); the partition census of `dst` again. With chunk_buckets the source is walked in chunks of that many
    buckets, each through all of these steps, with a host read of each chunk's summary count as well.
    Returns delta_resync()'s fields -- the install counts {raised, equal, older, missed} (and inserted, replaced,
    evictions with insert), records (the records fetched and installed: needed), scanned_keys, partitions,
    differing_before, differing_after, unresolved -- plus summaries, needed, classes (the six class counts of the
    need pass by name) and the bytes shipped: bytes_summaries = 16 summaries, bytes_keys = 8 needed, bytes_records =
    E needed, beside bytes_partition_delta = E summaries, what delta_resync() ships for the same partitions.
    The need list holds the keys `dst` lacks without saying which they are, so they are fetched too; without
    insert their records are `missed` by the install, as in delta_resync(). Every limit of a repair holds: `dst` is
    quiet meanwhile, no tables with RMWs, nobody is re-admitted to the membership, and a partition that still
    differs is reported in unresolved, never hidden (`dst` newer in a key: class `older`; a key it lacks, without
    insert: `missed`; keys lost to `replaced` / `evictions` with it)."""
    assert dst.sizes == src.sizes, "records of one entry size only"
    if part_bits is None:
        part_bits = min(20, _log2_buckets(min(src.cfg.num_bkts, dst.cfg.num_bkts)))
    part_bits = int(part_bits)
    dev = torch.device("cuda", src.device)
    E = src.sizes.entry
    rows = src.census_parts(part_bits).tensor
    mask, count = part_diff(rows, dst.census_parts(part_bits))
    n, differing = _selected_keys(rows, mask, count)
    sink = _RecordSink(dst, insert, dev)
    classes = torch.zeros(6, dtype=torch.int64, device=dev)
    absent = torch.zeros(1, dtype=torch.int64, device=dev)
    summaries = scanned = needed = 0
    if n:
        chunks = _bucket_chunks(src.cfg.num_bkts, chunk_buckets)
        sbuf = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        kbuf = torch.empty(max(n, 2), dtype=torch.int64, device=dev)
        for lo, hi in chunks:
            sm = src.summaries((lo, hi), part_bits=part_bits, part_mask=mask, out=sbuf)
            # (the whole table at once: its summary count is n, checked with the read of `needed` below)
            m = n if len(chunks) == 1 else sm.records
            nd = dst.need(sm, n=m, out=kbuf[:max(m, 1)])
            h = [int(v) for v in torch.cat([sm.result, nd.result]).cpu().tolist()]
            assert h[0] == m, "the selected partitions' key counts are the summaries' count"
            summaries, scanned, k = summaries + h[0], scanned + h[1], h[2 + 6]
            classes += nd.result[:6]
            needed += k
            if k:
                f = src.fetch(nd, n=k)
                absent += f.result[1:2]
                sink(f.tensor, k)
        assert summaries == n, "the selected partitions' key counts are the summaries' count"
        assert int(absent.cpu()[0]) == 0, "the source does not hold a key it summarised"
    out = sink.result()
    out.update(records=needed, scanned_keys=scanned, partitions=1 << part_bits, differing_before=differing,
               summaries=summaries, needed=needed, classes=dict(zip(NEED_CLASSES, (int(v) for v in classes.cpu().tolist()))))
    out.update(_key_delta_bytes(E, summaries, needed))
    out.update(_delta_verify(dst, rows, part_bits))
    return out


def group_key_delta_resync(kvs: HermesKV, group, source_rank: int, stale_ranks, part_bits: int | None,
                           chunk_buckets: int | None, insert: bool = False) -> dict:
    """key_delta_resync() across ranks. Collective: every rank of `group` calls it with the same arguments and its
    own table (tables of one entry size; bucket counts may differ). Rows, masks and the summary count as in
    group_delta_resync(): the source broadcasts its partition rows, each stale rank diffs them against its own, the
    masks are united (all_reduce MAX). Then, per chunk of chunk_buckets buckets of the source (default: the whole
    table): the source broadcasts its summaries of the united partitions; each stale rank computes its need list;
    the lists reach the source padded to the longest (an all_reduce MAX of the counts, read on the host, then one
    all_gather of count + keys); the source fetches the unique union of them (torch.unique) once and broadcasts
    its size and the records; every stale rank installs them (insert=True: upserts). A record only another rank
    needed is `equal` or `older` here and does no harm, the install being timestamp-guarded.
    Returns this rank's install counts (zeros where it did not install), records (the union's size), scanned_keys,
    partitions, selected, summaries, this rank's needed and classes (zeros where it is not stale), the bytes the
    source broadcast (bytes_summaries, bytes_records = E records), bytes_keys = 8 x this rank's needed, beside
    bytes_partition_delta = E summaries, and this rank's differing_before, differing_after and unresolved. The
    conditions are key_delta_resync()'s: a stale rank takes no client operations meanwhile, no tables with RMWs,
    nobody is re-admitted to the membership here, and a partition that still differs is reported in unresolved."""
    import torch.distributed as dist
    rank = dist.get_rank(group)
    world = dist.get_world_size(group)
    src = dist.get_global_rank(group, source_rank) if group is not None else int(source_rank)
    stale = {int(r) for r in stale_ranks}
    assert source_rank not in stale
    dev = torch.device("cuda", kvs.device)
    E = kvs.sizes.entry
    geo = torch.tensor([kvs.cfg.num_bkts, _log2_buckets(kvs.cfg.num_bkts)], dtype=torch.int64, device=dev)
    low = geo[1:].clone()
    dist.broadcast(geo, src, group=group)
    dist.all_reduce(low, op=dist.ReduceOp.MIN, group=group)
    num_bkts, most_bits = int(geo[0].cpu()), int(low.cpu()[0])
    part_bits = min(20, most_bits) if part_bits is None else int(part_bits)
    assert part_bits <= most_bits, "part_bits above log2 of a rank's bucket count"
    P = 1 << part_bits
    mine = kvs.census_parts(part_bits).tensor
    rows = mine.clone()
    dist.broadcast(rows, src, group=group)
    mask = torch.zeros(P, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    if rank in stale:
        mask, count = part_diff(rows, mine)
    differing = count.clone()
    dist.all_reduce(mask, op=dist.ReduceOp.MAX, group=group)
    n, selected = _selected_keys(rows, mask, (mask != 0).sum().reshape(1))
    sink = _RecordSink(kvs, insert, dev)
    classes = torch.zeros(6, dtype=torch.int64, device=dev)
    summaries = scanned = needed = records = 0
    if n:
        sbuf = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        for lo, hi in _bucket_chunks(num_bkts, chunk_buckets):
            if rank == source_rank:
                res = kvs.summaries((lo, hi), part_bits=part_bits, part_mask=mask, out=sbuf).result
            dist.broadcast(res, src, group=group)
            m, sc = (int(v) for v in res.cpu().tolist())
            assert summaries + m <= n, "more summaries than the selected partitions' keys"
            summaries, scanned = summaries + m, scanned + sc
            if not m:
                continue
            dist.broadcast(sbuf[:m * 16], src, group=group)
            # this rank's need list, then the longest list's length (every rank reads it: it sizes the gather)
            k = torch.zeros(1, dtype=torch.int64, device=dev)
            nd = None
            if rank in stale:
                nd = kvs.need(sbuf, n=m)
                classes += nd.result[:6]
                k = nd.result[6:7].clone()
            most = k.clone()
            dist.all_reduce(most, op=dist.ReduceOp.MAX, group=group)
            k_host, most_host = (int(v) for v in torch.cat([k, most]).cpu().tolist())
            needed += k_host
            if not most_host:
                continue
            send = torch.zeros(1 + most_host, dtype=torch.int64, device=dev)   # count, keys, padding
            send[0:1] = k
            if k_host:
                send[1:1 + k_host] = nd.keys[:k_host]
            lists = torch.empty(world * (1 + most_host), dtype=torch.int64, device=dev)
            dist.all_gather_into_tensor(lists, send, group=group)
            u = torch.zeros(1, dtype=torch.int64, device=dev)
            rbuf = None
            if rank == source_rank:
                counts = [int(c) for c in lists.view(world, -1)[:, 0].cpu().tolist()]
                union = torch.unique(torch.cat([lists.view(world, -1)[r, 1:1 + c] for r, c in enumerate(counts)]))
                f = kvs.fetch(union.contiguous())
                assert f.absent == 0, "the source does not hold a key it summarised"
                rbuf, u[0] = f.tensor, union.numel()
            dist.broadcast(u, src, group=group)
            u_host = int(u.cpu()[0])
            if rbuf is None:
                rbuf = torch.empty(u_host * E, dtype=torch.uint8, device=dev)
            dist.broadcast(rbuf, src, group=group)
            records += u_host
            if rank in stale:
                sink(rbuf, u_host)
    out = sink.result()
    out.update(records=records, scanned_keys=scanned, partitions=P, selected=selected, summaries=summaries,
               needed=needed, classes=dict(zip(NEED_CLASSES, (int(v) for v in classes.cpu().tolist()))),
               differing_before=int(differing.cpu()[0]))
    out.update(_key_delta_bytes(E, summaries, needed))
    out["bytes_records"] = E * records
    out.update(_delta_verify(kvs, rows, part_bits) if rank in stale else {"differing_after": 0, "unresolved": []})
    return out


def default_sub_cells(differing_partitions: int) -> int:
    """a sketch-level repair's default S: 3 S >= 2.0 x (two elements per differing partition, the two versions of one
    key), floor 32 -- 128 bytes of sketch per differing partition"""
    return max(32, -(-4 * int(differing_partitions) // 3))


def _fold_selected(kvs: HermesKV, part_bits: int, mask: torch.Tensor, n: int, S: int, chunk_buckets, dev):
    """(the sketch of the table's summaries of the selected partitions, folded chunk by chunk into one sketch, and
    [summaries, scanned keys] summed on the device). n: the table's key count in those partitions, which sizes the
    summary buffer; with several chunks each chunk's count is read on the host."""
    from .kvs import sketch
    sk = None
    tot = torch.zeros(2, dtype=torch.int64, device=dev)
    sbuf = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=dev)
    chunks = _bucket_chunks(kvs.cfg.num_bkts, chunk_buckets) if n else []
    for lo, hi in chunks:
        sm = kvs.summaries((lo, hi), part_bits=part_bits, part_mask=mask, out=sbuf)
        tot += sm.result
        sk = sketch(sm, S, n=n if len(chunks) == 1 else sm.records, out=sk, accumulate=sk is not None)
    if sk is None:
        sk = sketch(sbuf, S, n=0)
    return sk, tot


def _key_level_exchange(dst: HermesKV, src: HermesKV, part_bits: int, mask: torch.Tensor, n: int, chunk_buckets,
                        sink: _RecordSink, dev) -> tuple:
    """key_delta_resync()'s exchange for the selected partitions: per chunk the source's summaries, the target's
    need list, the source's fetch, the records into `sink`. Returns (summaries, scanned, needed, classes tensor)."""
    classes = torch.zeros(6, dtype=torch.int64, device=dev)
    absent = torch.zeros(1, dtype=torch.int64, device=dev)
    summaries = scanned = needed = 0
    if n:
        chunks = _bucket_chunks(src.cfg.num_bkts, chunk_buckets)
        sbuf = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        kbuf = torch.empty(max(n, 2), dtype=torch.int64, device=dev)
        for lo, hi in chunks:
            sm = src.summaries((lo, hi), part_bits=part_bits, part_mask=mask, out=sbuf)
            m = n if len(chunks) == 1 else sm.records
            nd = dst.need(sm, n=m, out=kbuf[:max(m, 1)])
            h = [int(v) for v in torch.cat([sm.result, nd.result]).cpu().tolist()]
            assert h[0] == m, "the selected partitions' key counts are the summaries' count"
            summaries, scanned, k = summaries + h[0], scanned + h[1], h[2 + 6]
            classes += nd.result[:6]
            needed += k
            if k:
                f = src.fetch(nd, n=k)
                absent += f.result[1:2]
                sink(f.tensor, k)
        assert summaries == n, "the selected partitions' key counts are the summaries' count"
        assert int(absent.cpu()[0]) == 0, "the source does not hold a key it summarised"
    return summaries, scanned, needed, classes


def sketch_delta_resync(dst: HermesKV, src: HermesKV, part_bits: int | None = None, chunk_buckets: int | None = None,
                        insert: bool = False, sub_cells: int | None = None) -> dict:
    """key_delta_resync() that ships an invertible sketch where it ships summaries (include/hermeskv.h,
    "Sketch-level delta repair"), both tables in this process. In this order: both partition censuses and
    part_diff, as delta_resync(); one host read of both tables' key counts in the differing partitions and of the
    number of those partitions; HermesKV.summaries of `src` and of `dst` for those partitions, the same mask on
    both, each folded into one sketch of S = sub_cells cells per subtable (default default_sub_cells(differing
    partitions)) -- with chunk_buckets each table is walked in chunks of that many of its own buckets, all folded
    into the one sketch; sketch_decode(source's sketch, target's sketch), "at dst"; one host read of its result;
    HermesKV.need of `dst` on only_a, the summaries only the source holds; one host read of `needed`;
    HermesKV.fetch from `src`; install into `dst` (insert=True: upsert); the partition census of `dst` again.
    When the decode is not complete (undecoded != 0, or more elements than the lists hold) the partial lists are
    dropped and key_delta_resync()'s exchange runs instead: the source's summaries go to need.
    Returns key_delta_resync()'s fields -- there `summaries` is the source's key count in the differing partitions
    and bytes_summaries = 16 summaries what the key-level repair ships for them (and what was shipped after a
    fallback); classes counts the summaries that reached need: only_src of them, or all after a fallback -- plus
    sub_cells, only_src, only_dst (the decode's counts; only_dst is returned for a two-way repair and not used),
    undecoded, passes, fallback, and bytes_sketch = 96 sub_cells, the sketch that crosses. Every limit of a repair
    holds unchanged: `dst` is quiet meanwhile, no tables with RMWs, nobody is re-admitted to the membership, and a
    partition that still differs is reported in unresolved, never hidden."""
    from .kvs import sketch_decode
    assert dst.sizes == src.sizes, "records of one entry size only"
    if part_bits is None:
        part_bits = min(20, _log2_buckets(min(src.cfg.num_bkts, dst.cfg.num_bkts)))
    part_bits = int(part_bits)
    dev = torch.device("cuda", src.device)
    E = src.sizes.entry
    rows = src.census_parts(part_bits).tensor
    rows_dst = dst.census_parts(part_bits).tensor
    mask, count = part_diff(rows, rows_dst)
    sel = mask != 0
    n, n_dst, differing = (int(v) for v in torch.stack([(rows[:, 2] * sel).sum(), (rows_dst[:, 2] * sel).sum(),
                                                        count[0]]).cpu().tolist())
    S = default_sub_cells(differing) if sub_cells is None else int(sub_cells)
    sink = _RecordSink(dst, insert, dev)
    classes = torch.zeros(6, dtype=torch.int64, device=dev)
    scanned = needed = 0
    dec = dict.fromkeys(("only_a", "only_b", "undecoded", "passes"), 0)
    fallback = False
    if differing:
        sk_src, tot_src = _fold_selected(src, part_bits, mask, n, S, chunk_buckets, dev)
        sk_dst, tot_dst = _fold_selected(dst, part_bits, mask, n_dst, S, chunk_buckets, dev)
        d = sketch_decode(sk_src, sk_dst)
        h = [int(v) for v in torch.cat([d.result[:4], tot_src, tot_dst]).cpu().tolist()]
        dec = dict(zip(dec, h[:4]))
        assert h[4] == n and h[6] == n_dst, "the selected partitions' key counts are the summaries' counts"
        scanned = h[5]
        fallback = dec["undecoded"] != 0 or dec["only_a"] > 3 * S or dec["only_b"] > 3 * S
        if fallback:
            _, sc, needed, classes = _key_level_exchange(dst, src, part_bits, mask, n, chunk_buckets, sink, dev)
            scanned += sc
        elif dec["only_a"]:
            nd = dst.need(d.only_a, n=dec["only_a"])
            classes = nd.result[:6]
            needed = nd.needed
            if needed:
                f = src.fetch(nd, n=needed)
                sink(f.tensor, needed)
                assert f.absent == 0, "the source does not hold a key it summarised"
    out = sink.result()
    out.update(records=needed, scanned_keys=scanned, partitions=1 << part_bits, differing_before=differing,
               summaries=n, needed=needed, classes=dict(zip(NEED_CLASSES, (int(v) for v in classes.cpu().tolist()))))
    out.update(_key_delta_bytes(E, n, needed))
    out.update(sub_cells=S, only_src=dec["only_a"], only_dst=dec["only_b"], undecoded=dec["undecoded"],
               passes=dec["passes"], fallback=fallback, bytes_sketch=96 * S)
    out.update(_delta_verify(dst, rows, part_bits))
    return out


def _group_need_exchange(kvs: HermesKV, group, src: int, is_source: bool, is_stale: bool, nd, sink: _RecordSink,
                         dev) -> tuple:
    """group_key_delta_resync()'s second half for one need list per stale rank (nd None elsewhere): the lists
    reach the source padded to the longest, the source fetches their unique union once and broadcasts the records,
    the stale ranks take them into `sink`. Returns (this rank's needed, the union's size)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    E = kvs.sizes.entry
    k = nd.result[6:7].clone() if nd is not None else torch.zeros(1, dtype=torch.int64, device=dev)
    most = k.clone()
    dist.all_reduce(most, op=dist.ReduceOp.MAX, group=group)
    k_host, most_host = (int(v) for v in torch.cat([k, most]).cpu().tolist())
    if not most_host:
        return k_host, 0
    send = torch.zeros(1 + most_host, dtype=torch.int64, device=dev)   # count, keys, padding
    send[0:1] = k
    if k_host:
        send[1:1 + k_host] = nd.keys[:k_host]
    lists = torch.empty(world * (1 + most_host), dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(lists, send, group=group)
    u = torch.zeros(1, dtype=torch.int64, device=dev)
    rbuf = None
    if is_source:
        counts = [int(c) for c in lists.view(world, -1)[:, 0].cpu().tolist()]
        union = torch.unique(torch.cat([lists.view(world, -1)[r, 1:1 + c] for r, c in enumerate(counts)]))
        f = kvs.fetch(union.contiguous())
        assert f.absent == 0, "the source does not hold a key it summarised"
        rbuf, u[0] = f.tensor, union.numel()
    dist.broadcast(u, src, group=group)
    u_host = int(u.cpu()[0])
    if rbuf is None:
        rbuf = torch.empty(u_host * E, dtype=torch.uint8, device=dev)
    dist.broadcast(rbuf, src, group=group)
    if is_stale:
        sink(rbuf, u_host)
    return k_host, u_host


def group_sketch_delta_resync(kvs: HermesKV, group, source_rank: int, stale_ranks, part_bits: int | None,
                              chunk_buckets: int | None, insert: bool = False, sub_cells: int | None = None) -> dict:
    """sketch_delta_resync() across ranks, on group_key_delta_resync()'s choreography. Collective: every rank of
    `group` calls it with the same arguments and its own table. Rows, masks and the source's key count as there: the
    source broadcasts its partition rows, each stale rank diffs them against its own, the masks are united. Then
    the source and every stale rank fold their own summaries of the united partitions into a sketch of S =
    sub_cells cells per subtable (default default_sub_cells(partitions in the union)); the source broadcasts its
    sketch, 96 S bytes; each stale rank decodes it against its own; an all_reduce MAX of `undecoded` (with a list
    overflow counted as undecoded) decides the fallback for the whole call, so every rank takes the same branch.
    Without it each stale rank's need list comes from its only_a; the lists reach the source, which fetches their
    unique union once and broadcasts the records, as in group_key_delta_resync(). With it that function's exchange
    runs per chunk: the source's summaries are broadcast and go to need.
    Returns group_key_delta_resync()'s fields (summaries: the source's key count in the united partitions;
    bytes_summaries what a key-level repair broadcasts for them, and what was broadcast after a fallback) plus
    sub_cells, this rank's only_src, only_dst, undecoded and passes (zeros where it is not stale), fallback, and
    bytes_sketch = 96 sub_cells. The conditions are sketch_delta_resync()'s."""
    import torch.distributed as dist
    from .kvs import Sketch, sketch_decode
    rank = dist.get_rank(group)
    src = dist.get_global_rank(group, source_rank) if group is not None else int(source_rank)
    stale = {int(r) for r in stale_ranks}
    assert source_rank not in stale
    is_source, is_stale = rank == source_rank, rank in stale
    dev = torch.device("cuda", kvs.device)
    E = kvs.sizes.entry
    geo = torch.tensor([kvs.cfg.num_bkts, _log2_buckets(kvs.cfg.num_bkts)], dtype=torch.int64, device=dev)
    low = geo[1:].clone()
    dist.broadcast(geo, src, group=group)
    dist.all_reduce(low, op=dist.ReduceOp.MIN, group=group)
    num_bkts, most_bits = int(geo[0].cpu()), int(low.cpu()[0])
    part_bits = min(20, most_bits) if part_bits is None else int(part_bits)
    assert part_bits <= most_bits, "part_bits above log2 of a rank's bucket count"
    P = 1 << part_bits
    mine = kvs.census_parts(part_bits).tensor
    rows = mine.clone()
    dist.broadcast(rows, src, group=group)
    mask = torch.zeros(P, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    if is_stale:
        mask, count = part_diff(rows, mine)
    differing = count.clone()
    dist.all_reduce(mask, op=dist.ReduceOp.MAX, group=group)
    sel = mask != 0
    n, n_own, selected = (int(v) for v in torch.stack([(rows[:, 2] * sel).sum(), (mine[:, 2] * sel).sum(),
                                                       sel.sum()]).cpu().tolist())
    S = default_sub_cells(selected) if sub_cells is None else int(sub_cells)
    sink = _RecordSink(kvs, insert, dev)
    classes = torch.zeros(6, dtype=torch.int64, device=dev)
    summaries = scanned = needed = records = 0
    dec = dict.fromkeys(("only_a", "only_b", "undecoded", "passes"), 0)
    fallback = False
    if selected:
        own = tot = None
        if is_source or is_stale:
            own, tot = _fold_selected(kvs, part_bits, mask, n_own, S, chunk_buckets, dev)
        cells = own.cells.clone() if is_source else torch.empty((3 * S, 4), dtype=torch.int64, device=dev)
        stats = tot.clone() if is_source else torch.zeros(2, dtype=torch.int64, device=dev)
        dist.broadcast(cells, src, group=group)
        dist.broadcast(stats, src, group=group)
        res = torch.zeros(4, dtype=torch.int64, device=dev)
        d = None
        if is_stale:
            d = sketch_decode(Sketch(cells, S), own)
            res = d.result[:4].clone()
        over = ((res[0:1] > 3 * S) | (res[1:2] > 3 * S)).to(torch.int64)
        und = torch.maximum(res[2:3], over)
        dist.all_reduce(und, op=dist.ReduceOp.MAX, group=group)
        h = [int(v) for v in torch.cat([res, und, stats]).cpu().tolist()]
        dec = dict(zip(dec, h[:4]))
        fallback = h[4] != 0
        assert h[5] == n, "the selected partitions' key counts are the summaries' count"
        summaries, scanned = n, h[6]
        if not fallback:
            nd = None
            if is_stale:
                nd = kvs.need(d.only_a, n=dec["only_a"])
                classes += nd.result[:6]
            needed, records = _group_need_exchange(kvs, group, src, is_source, is_stale, nd, sink, dev)
        elif n:
            summaries = 0
            sbuf = torch.empty(n * 16, dtype=torch.uint8, device=dev)
            sres = torch.zeros(2, dtype=torch.int64, device=dev)
            for lo, hi in _bucket_chunks(num_bkts, chunk_buckets):
                if is_source:
                    sres = kvs.summaries((lo, hi), part_bits=part_bits, part_mask=mask, out=sbuf).result
                dist.broadcast(sres, src, group=group)
                m, sc = (int(v) for v in sres.cpu().tolist())
                assert summaries + m <= n, "more summaries than the selected partitions' keys"
                summaries, scanned = summaries + m, scanned + sc
                if not m:
                    continue
                dist.broadcast(sbuf[:m * 16], src, group=group)
                nd = None
                if is_stale:
                    nd = kvs.need(sbuf, n=m)
                    classes += nd.result[:6]
                k, u = _group_need_exchange(kvs, group, src, is_source, is_stale, nd, sink, dev)
                needed, records = needed + k, records + u
    out = sink.result()
    out.update(records=records, scanned_keys=scanned, partitions=P, selected=selected, summaries=summaries,
               needed=needed, classes=dict(zip(NEED_CLASSES, (int(v) for v in classes.cpu().tolist()))),
               differing_before=int(differing.cpu()[0]))
    out.update(_key_delta_bytes(E, summaries, needed))
    out["bytes_records"] = E * records
    out.update(sub_cells=S, only_src=dec["only_a"], only_dst=dec["only_b"], undecoded=dec["undecoded"],
               passes=dec["passes"], fallback=fallback, bytes_sketch=96 * S)
    out.update(_delta_verify(kvs, rows, part_bits) if is_stale else {"differing_after": 0, "unresolved": []})
    return out


class LoopbackGroup:
    """N replicas driven phase by phase in one process; the collectives are tensor copies with
    exactly the layouts the RCCL driver produces (all-gather: row p = rank p's slab;
    all-to-all: row p of the output = row `rank` of rank p's input)."""

    def __init__(self, rounds: list[ReplicaRound], hades: bool = False, p2p: bool | None = None):
        """p2p (default: HKV_GROUP_P2P, on, as ReplicaGroupRound): INV slabs and ACK rows move peer by
        peer (row copies, `_rows`) and each replica applies its peers' INVs through the per-peer phases
        (invs_begin / invs_peer / invs_end) instead of the all-gather and all-to-all layouts."""
        self.rounds = rounds
        self.N = len(rounds)
        self.hades = hades
        self.p2p = (os.environ.get("HKV_GROUP_P2P", "1") != "0") if p2p is None else p2p
        self.plan = WidthPlan() if all(getattr(r, "packed_marshal", False) for r in rounds) else None
        self.hades_changes = []        # (round, rank, membership) of every agreed change
        self.clock = 0
        if hades:
            for r in rounds:
                r.hades_start()
            full = (1 << self.N) - 1
            for _ in range(16):        # spin_until_all_nodes_are_in_membership
                for r in rounds:
                    r.hades.update()
                exchange_views([r.hades for r in rounds])
                if all(r.hades.state()[0] == full for r in rounds):
                    break
            else:
                raise RuntimeError("Hades bootstrap did not reach the full membership")

    def _hades_period(self):
        rs = self.rounds
        res = {}
        for r in rs:
            if not r.failed:
                res[r.rank] = r.hades.update()
        exchange_views([None if r.failed else r.hades for r in rs])
        if any(ch for ch, _, _ in res.values()):
            for r in rs:
                ch, mb, _ = res.get(r.rank, (False, None, False))
                if ch:
                    self.hades_changes.append((self.clock, r.rank, mb))
                r.membership_change(membership=mb if ch else None)
            self._gather_io([r.val_total_io() for r in rs])
            w2 = max(r.val_width() for r in rs)
            self._gather_io([r.val_io(w2) for r in rs])
            for r in rs:
                r.vals(w2)

    @staticmethod
    def _gather(outs, ins):
        for o in outs:
            torch.cat([x.to(o.device) for x in ins], out=o)

    def _a2a(self, outs, ins):
        N = self.N
        for q, o in enumerate(outs):
            ov = o.view(N, -1)
            for p, x in enumerate(ins):
                ov[p].copy_(x.view(N, -1)[q])

    def _gather_io(self, ios):
        self._gather([o for o, _ in ios], [i for _, i in ios])

    @staticmethod
    def _rows(pairs):
        """pairs: (send, receive) of the per-peer exchanges, each receive the send's copy"""
        for snd, rcv in pairs:
            rcv.copy_(snd)

    def _a2a_io(self, ios):
        self._a2a([o for o, _ in ios], [i for _, i in ios])

    def step(self, drop: int | None = None, observer=None):
        """One round of every replica. observer(phase), when given, runs after each phase has
        finished on every replica ("local", "invs", "acks", "vals", "end"): property checks of
        the group's state between phases (tests)."""
        rs = self.rounds
        seen = observer or (lambda phase: None)
        steady = self.plan is not None and self.plan.steady(drop is not None or self.hades or
                                                            not all(r.unique_acks for r in rs))
        fold = steady and self.plan.fold
        for r in rs:
            if steady:
                r.own_total = None
                r.local(cap=self.plan.width)
            else:
                r.local()
        seen("local")
        if fold and self.p2p:   # the totals ride in the slabs' spare slots, taken per peer (invs_peer)
            width = self.plan.slab_width()
            shapes = [(width, None)] * len(rs)
            for r in rs:
                r.inv_io_total(width)
        elif fold:
            width = self.plan.slab_width()
            shapes = [(width, None)] * len(rs)
            self._gather_io([r.inv_io_total(width) for r in rs])
            for r in rs:
                r.take_inv_totals(width)
        elif steady:
            self._gather_io([r.inv_total_io() for r in rs])
            width = self.plan.slab_width()
            shapes = [(width, None)] * len(rs)
        else:
            self._gather_io([r.inv_total_io() for r in rs])
            shapes = [r.round_shape() for r in rs]
            width = shapes[0][0]                 # the same on every replica (max of the same totals)
            if self.plan is not None:
                self.plan.calibrate(width, rs[0].W * rs[0].C)
        N = self.N
        if self.p2p:   # row p of replica q's INVs: peer p's slab
            self._rows([(rs[p].inv_row_io(q, width)[0], rs[q].inv_row_io(p, width)[1])
                        for q in range(N) for p in range(N) if p != q])
        elif not fold:
            self._gather_io([r.inv_io(width) for r in rs])
        if drop is not None:
            for r in rs:
                r.peer_failing()
            rs[drop].fail()
        if self.p2p:
            for q, r in enumerate(rs):
                r.invs_begin(width)
                for p in range(N):
                    if p != q:
                        r.invs_peer(p, width, fold)
                r.invs_end(width)
        else:
            for r in rs:
                r.invs(width)
        seen("invs")
        if self.p2p:   # row p of replica q's ACKs: peer p's answers to q's INVs
            self._rows([(rs[p].ack_row_io(q, width)[0], rs[q].ack_row_io(p, width)[1])
                        for q in range(N) for p in range(N) if p != q])
        else:
            self._a2a_io([r.ack_io(width) for r in rs])
        for r, (_, stride) in zip(rs, shapes):
            r.acks(width, stride)
        seen("acks")
        if fold:
            self._gather_io([r.val_io_total(width) for r in rs])
            for r in rs:
                r.take_val_totals(width)
        else:
            self._gather_io([r.val_total_io() for r in rs])
            self._gather_io([r.val_io(width) for r in rs])
        for r in rs:
            r.vals(width)
        seen("vals")
        if self.hades:
            self._hades_period()
        elif drop is not None:
            for r in rs:
                r.membership_change(drop)
            self._gather_io([r.val_total_io() for r in rs])
            w2 = rs[0].val_width()
            self._gather_io([r.val_io(w2) for r in rs])
            for r in rs:
                r.vals(w2)
        for r in rs:
            r.refill()
        seen("end")
        self.clock += 1
