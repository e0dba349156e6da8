"""k_fastmcts against the plain CPython bandit loop (tests/fastmcts_reference.py, anchored
to the reference's records by tests/test_fastmcts_reference.py) at the shapes where its
two loops differ or hand over: the register path (roots of <= 128 children: lane / slot
layout, rewards pre-drawn up to a twist ahead, the generator position set back at the
end, DPP argmax) and the LDS path (> 128 children), slot boundary 64 / 65, path boundary
128 / 129, the maximum of 2048 children, iteration 1024 where the LDS copy of the log
table hands over to the global one, partial and empty searches, a NaN base (no draw),
and every kind of start position of the generator, odd ones included (a draw whose two
words straddle a twist).

Every field bk_fastmcts returns is compared: iterations, n_children, best_index, n_top,
top_index / top_visits / top_q up to n_top (beyond it the buffer is unspecified),
visits_out and all 625 words of the returned generator state.
Tolerance: exact everywhere (top_q as float64 by ==)."""
import math

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from tests import fastmcts_reference as R

pytestmark = pytest.mark.gpu
C = 1.414
BASE = 2.655
NAN = math.nan
LOG_ROWS = 5 * 2048 + 17 + 1  # the longest search below, + 1
LOGS = np.array([0.0] + [math.log(k) for k in range(1, LOG_ROWS)])  # as the agent's _log_table
FIELDS = ("iterations", "n_children", "best_index", "n_top", "top_index", "top_visits", "top_q", "visits_out",
          "state")

GRID_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 500, 2048)


def grid_iters(n):
    return sorted({0, 1, n - 1, n, n + 1, 2 * n + 5, n + 700, 1023 + n % 3, 1100})


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


def case(n, iters, pos, base, seed):
    return (n, iters, pos, base, seed)


def name(cs):
    n, iters, pos, base, _ = cs
    return f"(n={n}, iters={iters}, pos={pos}, base={base})"


def start_state(cs):
    return np.array(R.rng_at(cs[4], cs[2]).getstate()[1], dtype=np.uint32)


_WANT = {}


def want(cs):
    """The restatement's result for a case; computed once per module run, never modified."""
    key = tuple(repr(x) for x in cs)
    if key not in _WANT:
        n, iters, pos, base, seed = cs
        _WANT[key] = R.expected(n, iters, base, R.rng_at(seed, pos), C)
    return _WANT[key]


def record(out, vis, state):
    """One game's bk_fastmcts result as fastmcts_reference.expected() lays it out."""
    nt = int(out["n_top"])
    assert 0 <= nt <= N.FASTMCTS_TOP
    r = {"iterations": int(out["iterations"]), "n_children": int(out["n_children"]),
         "best_index": int(out["best_index"]), "n_top": nt, "top_index": out["top_index"][:nt].tolist(),
         "top_visits": out["top_visits"][:nt].tolist(), "top_q": out["top_q"][:nt].tolist(),
         "state": state.tolist()}
    if vis is not None:
        r["visits_out"] = vis.tolist()
    return r


def run(gpu, cases):
    """One launch, one wave per case."""
    mt = np.stack([start_state(cs) for cs in cases])
    ns = [cs[0] for cs in cases]
    out, vis = gpu.fastmcts(ns, [cs[1] for cs in cases], [cs[3] for cs in cases], mt, LOGS, C, want_visits=True)
    off = np.concatenate([[0], np.cumsum(ns)])
    return [record(out[i], vis[off[i]:off[i + 1]], mt[i]) for i in range(len(cases))]


def first_difference(got, exp, fields=FIELDS):
    """None, or a description of the first field (and element) where got != exp."""
    for f in fields:
        g, e = got[f], exp[f]
        if g == e:
            continue
        if isinstance(e, list):
            if len(g) != len(e):
                return f"{f}: length {len(g)}, expected {len(e)}"
            k = next(i for i in range(len(e)) if g[i] != e[i])
            return f"{f}[{k}]: {g[k]!r}, expected {e[k]!r}"
        return f"{f}: {g!r}, expected {e!r}"
    return None


def check(cases, got, fields=FIELDS):
    bad = []
    for cs, g in zip(cases, got):
        d = first_difference(g, want(cs), fields)
        if d is None and math.isnan(cs[3]) and g["state"] != start_state(cs).tolist():
            d = "state: changed although a NaN base draws nothing"
        if d is not None:
            bad.append(f"{name(cs)}: {d}")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from the CPython loop:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("base", [BASE, NAN], ids=["draws", "nan_base"])
def test_grid_matches_cpython_loop(gpu, base):
    """Children counts around every layout boundary x iteration counts of every class
    (none, one, partial, exactly expanded, first selection, a few rounds, past the LDS log
    table's 1024 rows), fresh generators (position 624), one seed per case."""
    cases = [case(n, it, 624, base, 1000 + 16 * i + j)
             for i, n in enumerate(GRID_N) for j, it in enumerate(grid_iters(n))]
    assert len(cases) >= 110 and {cs[0] for cs in cases} == set(GRID_N)
    check(cases, run(gpu, cases))


POSITIONS = (624, 0, 1, 2, 311, 621, 622, 623)


def test_generator_positions_match_cpython(gpu):
    """mt_state may stand at any position.  Odd ones reach the draw that straddles a
    twist (word 623, twist, word 0) on the register path: 623 at the first draw, 1 after
    311 pre-drawn rewards."""
    cases = [case(n, it, pos, BASE, 5000 + 100 * i + 10 * j + k)
             for i, n in enumerate((2, 64, 65, 128, 129, 193)) for j, it in enumerate((n + 37, 700))
             for k, pos in enumerate(POSITIONS)]
    got = run(gpu, cases)
    check(cases, got)
    # not vacuous: on each path an odd start whose returned position moved
    for lo, hi in ((1, 128), (129, 2048)):
        assert any(lo <= cs[0] <= hi and cs[2] % 2 == 1 and g["state"][624] != cs[2] for cs, g in zip(cases, got)), (lo, hi)


def test_search_ends_at_a_refill_boundary(gpu):
    """Searches whose LAST draw is special for the register path's pre-drawn rewards,
    where the position handed back comes from the rewind alone: the last draw is the
    straddling one (position 623 + 1 draw, 621 + 2, 1 + 312), the one just before it
    (1 + 311: an odd position comes back), the last of a whole twist's 312 (624 + 312,
    0 + 312: position 624 comes back, not yet twisted) and the first of the next twist
    (624 + 313).  One root per slot layout and one on the LDS path."""
    ends = ((623, 1), (621, 2), (1, 312), (1, 311), (624, 312), (0, 312), (624, 313), (622, 1), (622, 2))
    cases = [case(n, it, pos, BASE, 6000 + 20 * i + k)
             for i, n in enumerate((2, 64, 128, 129)) for k, (pos, it) in enumerate(ends)]
    got = run(gpu, cases)
    check(cases, got)
    assert {g["state"][624] for cs, g in zip(cases, got) if cs[0] <= 128} >= {1, 623, 624, 2}


def test_exact_ties_go_to_the_lower_child(gpu):
    """NaN base: all totals 0.0, so children of equal visits tie exactly and first-max
    must walk them in child order, round after round -- lane l slot 0 against lane l slot
    1, across the 16-lane rows, and across lanes' strided children on the LDS path.  The
    expected visits are the closed form, not the restatement."""
    cases = [case(n, 5 * n + 17, 624, NAN, 7000 + n) for n in (64, 65, 128, 129, 2048)]
    for cs, g in zip(cases, run(gpu, cases)):
        n, iters = cs[0], cs[1]
        by_child = R.round_robin_visits(n, iters)
        assert g["visits_out"] == by_child[::-1], name(cs)  # visits_out is by legal index n - 1 - child
        assert g["iterations"] == iters and g["n_children"] == n, name(cs)
        assert g["best_index"] == n - 1 and g["top_index"] == [n - 1 - j for j in range(10)], name(cs)
        assert g["top_q"] == [0.0] * 10, name(cs)
        assert g["state"] == start_state(cs).tolist(), name(cs)


MIXED = [case(2, 39, 623, BASE, 9001), case(64, 700, 1, 2.05, 9002), case(65, 65, 624, BASE, 9003),
         case(127, 0, 311, BASE, 9004), case(128, 1100, 622, 3.1, 9005), case(128, 300, 0, NAN, 9006),
         case(129, 1100, 623, BASE, 9007), case(130, 1, 2, 1.5, 9008), case(193, 230, 621, NAN, 9009),
         case(500, 1025, 1, 2.4, 9010), case(2048, 2100, 624, BASE, 9011), case(1, 12, 623, 0.75, 9012)]


def test_games_of_one_launch_are_independent(gpu):
    """Games of both paths with different sizes, counts, bases and positions in one launch
    give what each gives when launched alone (and both what the CPython loop gives)."""
    together = run(gpu, MIXED)
    check(MIXED, together)
    for cs, g in zip(MIXED, together):
        alone = run(gpu, [cs])[0]
        assert first_difference(alone, g) is None, f"{name(cs)}: {first_difference(alone, g)}"


def test_device_path_equals_host_path(gpu):
    """gpu.fastmcts_device (torch tensors, no staging copies) returns the host path's
    records and generator states."""
    import torch
    host = run(gpu, MIXED)
    ns = [cs[0] for cs in MIXED]
    iters = np.array([cs[1] for cs in MIXED], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    fo, fe = N.pow_half_fix(LOGS, rows=int(iters.max()))
    mt = np.stack([start_state(cs) for cs in MIXED])
    dev = torch.device("cuda", 0)
    d_mt = torch.from_numpy(mt.view(np.int32).copy()).to(dev)
    d_out = torch.zeros((len(MIXED), N.FASTMCTS_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    gpu.fastmcts_device(torch.from_numpy(off).to(dev), torch.from_numpy(iters).to(dev),
                        torch.tensor([cs[3] for cs in MIXED], dtype=torch.float64, device=dev), d_mt,
                        torch.from_numpy(LOGS).to(dev), torch.from_numpy(np.ascontiguousarray(fo)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(fe)).to(dev), C, d_out)
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy().view(N.FASTMCTS_OUT_DTYPE).reshape(-1)
    back = d_mt.cpu().numpy().view(np.uint32)
    fields = tuple(f for f in FIELDS if f != "visits_out")  # the device path returns none
    for i, cs in enumerate(MIXED):
        d = first_difference(record(out[i], None, back[i]), host[i], fields)
        assert d is None, f"{name(cs)}: {d}"
