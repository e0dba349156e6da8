"""The per-phase stencil class lists of csrc/orient_table.h (-DBK_STENCIL_MUX), evaluated
in Python integers.

BK_CLASS_LIST_MUX_P / _T / _U / _Q index a table of their own, BK_CLASS_TABLE_MUX_INIT.  For
every entry the class's term list is applied the way StencilClass::scan applies it -- term
0 and the terms with the zero flag unshifted, the others shifted right by their column
field of w1 -- with kind 1 read from the phase's second plane: p the horizontal pair
bc | bc >> 1, t the horizontal triple bc | bc >> 1 | bc >> 2, u the vertical triple
bc[r] | bc[r + 1] | bc[r + 2] and q the 2 x 2 square p[r] | p[r + 1], with a row past 19
absent.  The positions are those of
tests/test_stencil_table.py (random boards, the empty board with each start corner);
every anchor row must equal the brute-force fit-and-touch test of the orientation's cells.
Also: the 91 orientations appear exactly once across the phases, every column is <= 3, a
zero flag sits only on a column that is 0 in every entry of its class, and the lists'
anchor-row-weighted ORs + shifts equal what `gen_tables.py --mux-stats` counts (6,276
with p, t, u; 6,071 with q as well) and are fewer than the one-plane lists' 7,558.
Tolerance: exact.
"""
import importlib.util
import os
import re

import pytest

from tests import test_stencil_table as ST

PHASES = ("P", "T", "U", "Q")
ONE_PLANE_COST = 7558  # weighted NT + nz of the pair-plane-only cover (`--mux-stats`, phases p)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_tables", os.path.join(ST.ROOT, "tools", "gen_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mux():
    """({phase: [(i0, i1, h, toks)]}, [(w0, w1)] * 91, cells per g, info per g)"""
    with open(ST.HEADER) as f:
        text = f.read()
    lists = {}
    for ph in PHASES:
        rows = [tuple(int(x) for x in m.group(1).split(","))
                for m in re.finditer(r"X\(([^)]*)\)", ST._macro_body(text, "BK_CLASS_LIST_MUX_" + ph))]
        lists[ph] = [(r[0], r[1], r[2], r[3:]) for r in rows]
    table = [(int(a, 16), int(b, 16)) for a, b in
             re.findall(r"\{(0x[0-9a-f]+), (0x[0-9a-f]+)\}", ST._macro_body(text, "BK_CLASS_TABLE_MUX_INIT"))]
    cells_src = text[text.index("kOrientCellsHost"):text.index("kOrientIndexHost")]
    cells = [[(int(r), int(c)) for r, c in re.findall(r"\((\d+) << 8\) \| (\d+)", line)]
             for line in re.findall(r"\{([^{}]*)\},", cells_src)]
    info = [tuple(int(x) for x in m) for m in
            re.findall(r"(\d+) \| \((\d+) << 8\) \| \((\d+) << 16\) \| \((\d+) << 24\),\n", text)]
    assert len(table) == len(cells) == len(info) == 91
    return lists, table, cells, info


def _second_plane(bc, ph):
    if ph == "P":
        return [v | v >> 1 for v in bc]
    if ph == "T":
        return [v | v >> 1 | v >> 2 for v in bc]
    if ph == "U":
        return [bc[r] | (bc[r + 1] if r + 1 < 20 else 0) | (bc[r + 2] if r + 2 < 20 else 0) for r in range(20)]
    pair = [v | v >> 1 for v in bc]
    return [pair[r] | (pair[r + 1] if r + 1 < 20 else 0) for r in range(20)]


@pytest.fixture(scope="module")
def brute(mux):
    _lists, _table, cells, _info = mux
    out = []
    for own, occ, first, p in ST._positions():
        may, trig = ST._cell_sets(own, occ, first, p)
        bc = ST._planes(may, trig)[0]
        out.append(({ph: (bc, _second_plane(bc, ph)) for ph in PHASES},
                    [ST._brute_rows(cs, may, trig) for cs in cells]))
    assert sum(1 for _pl, rows in out for rws in rows if any(rws)) > 1000  # the positions have moves
    return out


def test_every_orientation_once_and_lists_contiguous(mux):
    lists, table, _cells, info = mux
    assert sorted(w0 >> 8 for w0, _ in table) == list(range(91))
    flat = [c for ph in PHASES for c in lists[ph]]
    assert flat[0][0] == 0 and flat[-1][1] == 91
    assert all(a[1] == b[0] for a, b in zip(flat, flat[1:]))  # every entry in one class of one phase
    for i0, i1, h, toks in flat:
        assert i0 < i1 and 1 <= len(toks) <= 5
        assert all(t & 3 in (0, 1) for t in toks)
        for i in range(i0, i1):
            w0, _w1 = table[i]
            pid, _n, gh, _gw = info[w0 >> 8]
            assert pid == w0 & 0xFF and gh == h, i
    print("orientations per phase:", {ph: sum(i1 - i0 for i0, i1, _h, _t in lists[ph]) for ph in PHASES})
    assert all(lists[ph] for ph in PHASES)


@pytest.mark.parametrize("ph", PHASES)
def test_phase_lists_compute_the_rule(mux, brute, ph):
    lists, table, _cells, _info = mux
    for i0, i1, h, toks in lists[ph]:
        for i in range(i0, i1):
            w0, w1 = table[i]
            g = w0 >> 8
            for pos, (planes, rows) in enumerate(brute):
                got = ST._scan(planes[ph], h, toks, w1)
                assert got == rows[g][:21 - h], (ph, i, g, pos)
                assert not any(rows[g][21 - h:])


def test_columns_and_zero_flags(mux):
    """Every shift is <= 3 (a shifted C bit reaches only B's off-board bits; w1 keeps 3
    bits per term) and nothing lies past the last term's field; term 0 carries no flag,
    and a flagged term's column is 0 in every entry of its class, where every column-0
    term is flagged (the classes are split by zero pattern)."""
    lists, table, _cells, _info = mux
    for ph in PHASES:
        for i0, i1, _h, toks in lists[ph]:
            assert not toks[0] & 4
            for i in range(i0, i1):
                w1 = table[i][1]
                assert w1 >> (3 * (len(toks) - 1)) == 0, (ph, i)
                for k in range(1, len(toks)):
                    col = (w1 >> (3 * (k - 1))) & 7
                    assert col <= 3, (ph, i, k)
                    assert bool(toks[k] & 4) == (col == 0), (ph, i, k)


def test_cost_is_what_the_generator_counts(mux, gen):
    """Weighted by anchor rows (21 - h): one OR-type op per term, one shift per unflagged
    term after term 0."""
    lists, _table, _cells, _info = mux
    cost = {}
    for ph in PHASES:
        nt = sum((21 - h) * len(toks) * (i1 - i0) for i0, i1, h, toks in lists[ph])
        nz = sum((21 - h) * sum(1 for k, t in enumerate(toks) if k > 0 and not t & 4) * (i1 - i0)
                 for i0, i1, h, toks in lists[ph])
        cost[ph] = (nt, nz)
    table = gen.orientations()
    stats = {ph.upper(): (nt, nz) for ph, _no, _npl, _nc, nt, nz in gen.mux_stats(table)}
    print("weighted (NT, nz) per phase:", cost)
    assert cost == stats
    total = sum(nt + nz for nt, nz in cost.values())
    assert total < ONE_PLANE_COST, total
    for phases, want in ((("p",), ONE_PLANE_COST), (("p", "t", "u"), 6276), (("p", "t", "u", "q"), 6071)):
        assert sum(nt + nz for _ph, _no, _npl, _nc, nt, nz in gen.mux_stats(table, phases)) == want, phases
    assert total == 6071
