"""The three playout hand-out modes (BK_TUNE_HANDOUT 0 / 1 / 2) play the same playouts.

bk_rollout's persistent grid gives playout ids to resident slots in one of three ways
(rollout_body in csrc/blokus_kernels.hip, chosen in the launcher): 0 = every slot pulls
from one counter; 1 = slot s plays s, s + nslots, s + 2 nslots, ...; 2 = slot s plays s,
then the first long_slots slots pull the rest.  "Results depend only on the playout id,
not on the slot" -- here with more than one resident round, which no other test has:
n just past one round (mode 2's wave-rounded long_slots), exactly two rounds, just past
two (the rest >= nslots branch of long_slots) and past three (a third and fourth round of
mode 1).  The handle is created with one block per CU so a round is
multi_processor_count x 256 slots and the sizes stay small; the roots are 40 moves into
the game so the playouts are short.  A sample over all rounds is compared with the
oracle's Philox replay.  Tolerance: exact (byte-identical records).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as O
from reinforcementlearning_blokus_amd import _native as N
from tests.helpers import oracle_fset, oracle_states, pack_many

pytestmark = pytest.mark.gpu

SEED = 20260307
BLOCK = 256  # threads per k_rollout / k_rollout_fr block


@pytest.fixture(scope="module")
def small_grid():
    """(handle with one resident block per CU, slots per round)."""
    import torch
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    with pytest.MonkeyPatch.context() as monkeypatch:
        monkeypatch.setenv("BK_BLOCKS_PER_CU", "1")
        monkeypatch.setenv("BK_FR_BLOCKS_PER_CU", "1")
        monkeypatch.delenv("BK_HANDOUT", raising=False)
        gpu = BlokusGPU(0)  # the library reads the environment once, when the handle is created
    return gpu, torch.cuda.get_device_properties(0).multi_processor_count * BLOCK


@pytest.fixture(scope="module")
def roots():
    boards = oracle_states(64, seed0=9100, lo=40, hi=40)
    st = pack_many(boards)
    assert (st["move_count"] == 40).all()
    return st, np.array([oracle_fset(b) for b in boards], dtype=N.FSET_DTYPE)


def _sizes(nslots):
    return [nslots + 1, nslots + 65, 2 * nslots, 2 * nslots + 1, 3 * nslots + 17]


def _sample(n, nslots):
    """About 100 playout ids spread over all rounds, with the ids either side of every
    round boundary and the last one."""
    ids = set(np.linspace(0, n - 1, 96).astype(np.int64).tolist())
    for k in range(1, (n + nslots - 1) // nslots):
        ids.update((k * nslots - 1, k * nslots))
    ids.update((0, n - 1))
    return sorted(i for i in ids if 0 <= i < n)


def _run_modes(gpu, launch, n, kernel):
    out = {}
    try:
        for mode in (0, 1, 2):
            gpu.tune(HANDOUT=mode)
            out[mode] = launch(n)
            assert gpu.last_kernel() == kernel
            gpu.synchronize()  # raises if the launch tripped its iteration guard
    finally:
        gpu.tune(HANDOUT=None)
    for mode in (0, 1, 2):
        assert out[mode].shape == (n,) and (out[mode]["status"] == 0).all(), mode
    for mode in (1, 2):
        diff = np.flatnonzero((out[mode].view(np.uint8).reshape(n, 32) !=
                               out[0].view(np.uint8).reshape(n, 32)).any(axis=1))
        assert not len(diff), (mode, len(diff), diff[:8].tolist())
    return out[0]


@pytest.mark.parametrize("which", range(5))
def test_handout_modes_equal_naive_order(small_grid, roots, which):
    """k_rollout at nslots + 1, nslots + 65, 2 nslots, 2 nslots + 1 and 3 nslots + 17."""
    gpu, nslots = small_grid
    st, _ = roots
    n = _sizes(nslots)[which]
    idx = (np.arange(n) % len(st)).astype(np.int32)
    res = _run_modes(gpu, lambda k: gpu.rollout(st, k, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED,
                                                root_index=idx), n, "k_rollout")
    assert (res["plies"] > 0).any() and (res["plies"] <= 84 - 40).all()
    ost = (O.State * len(st)).from_buffer_copy(st.tobytes())

    def one(pid):
        r, _ = O.playout_arena_philox(O.unpack(ost[int(idx[pid])]), SEED, pid, O.ORDER_NAIVE)
        return pid, bytes(r)

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(one, _sample(n, nslots)))
    bad = [pid for pid, rb in refs if res[pid].tobytes() != rb]
    assert len(refs) >= 96 and not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("which", [3, 4])
def test_handout_modes_equal_frontier_order(small_grid, roots, which):
    """k_rollout_fr (hand-out 0 by default) at 2 nslots + 1 and 3 nslots + 17."""
    gpu, nslots = small_grid
    st, fs = roots
    n = _sizes(nslots)[which]
    idx = (np.arange(n) % len(st)).astype(np.int32)
    res = _run_modes(gpu, lambda k: gpu.rollout_frontier(st, fs, k, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX,
                                                         seed=SEED, root_index=idx), n, "k_rollout_fr")

    def one(pid):
        b = O.board_from(st[int(idx[pid])].tobytes(), fs[int(idx[pid])])
        r, _ = O.playout_arena_philox(b, SEED, pid, O.ORDER_FRONTIER)
        return pid, bytes(r)

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(one, _sample(n, nslots)))
    bad = [pid for pid, rb in refs if res[pid].tobytes() != rb]
    assert len(refs) >= 96 and not bad, (len(bad), bad[:8])
