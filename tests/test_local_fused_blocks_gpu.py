"""The fused local pass (k_local_fused) around its 64-element blocks, byte for byte against the oracle.

Two waves stage 32 elements each; one wave then resolves all 64 on the LDS copies, a key's first writer (F) runs its
exec function on its own LDS copy of the entry, and the wave stores the finished images to the first writers' shadows
four lanes per image, 16 images per step. The cases (tests/local_block_cases.py; tests/test_local_fused_blocks_cpu.py
shows on the oracle alone that each produces its outcome) put launch ends, counts, patches, F, deferred elements,
misses and skipped elements at the first and last position of each half of a block, and 0 to 64 first writers into
one block. Every case runs on a LOG table and on an INLINE-preferred one whose table is compared where the case says
so (a deferred Mirror: ops, state mirror and error flags per launch), at skew 0 and 3, on the multi-kernel engine.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests import local_block_cases as B  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
VARIANTS = [(LOG, 0), (LOG, 3), (INLINE, 0), (INLINE, 3)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def engine_path():
    """The multi-kernel engine for every launch: left to itself a launch this small takes the single-workgroup kernel"""
    from hermes_amd import kvs
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
    yield
    kvs.HermesKV.default_flags = 0


class BlockGpuEngine(GpuEngine):
    """GpuEngine whose local launches may carry patches (and then the opcode mirror of the patched ops, as the bench
    round's do): the Mirror applies them to the oracle's input and compares the patched ops after the launch."""

    def launch(self, btype, elems, n_batches, stride, mb, patch=None, **kw):
        if patch is None:
            return super().launch(btype, elems, n_batches, stride, mb, **kw)
        want = elems.copy()
        want.view(np.uint8)[...] = elems.view(np.uint8)
        B.apply_patches(want.view(np.uint8).reshape(len(want), -1), patch, self.sizes.st_value)
        extra = {"patch": torch.from_numpy(patch.reshape(-1).copy()).cuda(),
                 "opcode_in": torch.from_numpy(want["opcode"].copy()).cuda()}
        real = self.m.batch
        self.m.batch = lambda *a, **k: real(*a, **extra, **k)
        try:
            return super().launch(btype, elems, n_batches, stride, mb, **kw)
        finally:
            self.m.batch = real


def make_pair(layout, skew, what):
    from hermes_amd.kvs import HermesKV
    n_keys, bkts, cap = C.GEO["S"]
    g = HermesKV(n_keys, bkts, cap, machine_id=0, skew=skew)
    o = C.make_oracle("S", skew=skew)
    T = C.describe(o, "S")
    if layout == INLINE:
        assert g.prefer_layout(INLINE)
    m = Mirror(g, o, f"{what} layout {layout} skew {skew}", table_check="deferred")
    return g, m, BlockGpuEngine(m, layout=layout == INLINE), T


def finish(g, m, layout, launches):
    lay = g.layout()
    assert m.launches == launches, (m.launches, launches)
    assert lay["inline_launches"] == (launches if layout == INLINE else 0), lay
    assert g.take_error_flags() == 0


@pytest.mark.parametrize("layout,skew", VARIANTS)
def test_block_edges(layout, skew):
    """launches of 1 to 200 elements (ends at 31, 32, 33, 63, 64, 65 of a block; 3 x 43 and 2 x 100), each with and
    without counts (one ending inside wave 0's half, one 0) and with and without patches at positions 0, 31, 32, 63"""
    g, m, eng, T = make_pair(layout, skew, "edges")
    facts = B.case_block_edges(eng, T, skew=skew)
    assert any(f[2] and B.PUT_SUCCESS in f[3]["state"][f[5]] for f in facts), "a patched PUT wrote"
    finish(g, m, layout, 4 * len(B.SIZES))


@pytest.mark.parametrize("layout,skew", VARIANTS)
def test_first_writer_position(layout, skew):
    """F at block position 0, 31, 32, 63, its key's GETs and PUTs before and after it in both halves; an inline key and
    its bucket-mate"""
    g, m, eng, T = make_pair(layout, skew, "first writer position")
    facts = B.case_first_writer_position(eng, T, skew=skew)
    assert all(after[p] == B.PUT_SUCCESS for p, _, _, _, after in facts)
    finish(g, m, layout, 2 * len(B.EDGE))


@pytest.mark.parametrize("layout,skew", VARIANTS)
def test_first_writers_per_block(layout, skew):
    """0, 1, 16, 17, 33 and 64 first writers in one block: the image stores run no step, one, two, three and four"""
    g, m, eng, T = make_pair(layout, skew, "first writers per block")
    facts = B.case_first_writers_per_block(eng, T, skew=skew)
    assert [int((after == B.PUT_SUCCESS).sum()) for _, _, after in facts] == list(B.FIRST_WRITERS)
    finish(g, m, layout, len(B.FIRST_WRITERS))


@pytest.mark.parametrize("layout,skew", VARIANTS)
def test_deferred(layout, skew):
    """1, 2 and 64 elements of a block on keys a unique INV launch left INVALID, GETs that replay among them: they
    wait for k_local_deferred, the block's other elements resolve in the fused pass"""
    g, m, eng, T = make_pair(layout, skew, "deferred")
    facts = B.case_deferred(eng, T, skew=skew)
    assert all(B.REPLAY_SUCCESS in after for _, _, _, after in facts)
    finish(g, m, layout, 1 + len(B.DEFERRED))


@pytest.mark.parametrize("layout,skew", VARIANTS)
def test_misses_and_skipped(layout, skew):
    """absent keys and skipped elements in both halves of a block and in a partial last block"""
    g, m, eng, T = make_pair(layout, skew, "misses and skipped")
    miss, skipped, before, after = B.case_misses_and_skipped(eng, T, skew=skew)
    assert (after["state"][miss] == B.MISS).all()
    finish(g, m, layout, 1)
