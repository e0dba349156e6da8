"""The stencil class lists of csrc/orient_table.h, evaluated in Python integers.

For every table entry (all 91 orientations) the class's term list is applied the way
StencilClass::scan applies it -- term 0 and the terms with the zero flag unshifted, the
others shifted right by their column field of w1 -- to the blocked / corner planes of a
few dozen random 20 x 20 positions and of the empty board with each seat's start corner.
Every anchor row must equal a brute-force fit-and-touch test of the orientation's cells
on the grid.  All three lists over the one table are checked: the default one (classes
split by zero pattern), the unsplit one with the shared flags (BK_STENCIL_COMMON) and the
unflagged one (BK_STENCIL_PLAIN).  A zero flag may sit only where the column is 0 in every
entry of the class, and the committed header must be the generator's output.  Tolerance:
exact.
"""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "reinforcementlearning_blokus_amd", "csrc", "orient_table.h")
M32 = 0xFFFFFFFF
OFFBOARD = 0xFFF00000


def _macro_body(text, name):
    m = re.search(r"#define " + name + r"\b[^\n]*\\\n((?:.*\\\n)*)", text)
    assert m, name
    return m.group(1)


@pytest.fixture(scope="module")
def header():
    with open(HEADER) as f:
        text = f.read()
    lists = {}
    for name in ("BK_CLASS_LIST_ZERO", "BK_CLASS_LIST_COMMON", "BK_CLASS_LIST_PLAIN"):
        rows = [tuple(int(x) for x in m.group(1).split(","))
                for m in re.finditer(r"X\(([^)]*)\)", _macro_body(text, name))]
        lists[name] = [(r[0], r[1], r[2], r[3:]) for r in rows]
    table = [(int(a, 16), int(b, 16))
             for a, b in re.findall(r"\{(0x[0-9a-f]+), (0x[0-9a-f]+)\}", _macro_body(text, "BK_CLASS_TABLE_INIT"))]
    cells_src = text[text.index("kOrientCellsHost"):text.index("kOrientIndexHost")]
    cells = []
    for line in re.findall(r"\{([^{}]*)\},", cells_src):
        vals = re.findall(r"\((\d+) << 8\) \| (\d+)", line)
        cells.append([(int(r), int(c)) for r, c in vals])
    info = [tuple(int(x) for x in m) for m in
            re.findall(r"(\d+) \| \((\d+) << 8\) \| \((\d+) << 16\) \| \((\d+) << 24\),\n", text)]
    assert len(table) == len(cells) == len(info) == 91
    for (_pid, n, _h, _w), cs in zip(info, cells):
        assert len(cs) == n
    return text, lists, table, cells, info


def _positions():
    """[(own bool[20,20], occupied bool[20,20], first, player)]"""
    rng = np.random.RandomState(20260311)
    out = []
    for i in range(36):
        k = int(round((0.03, 0.08, 0.15, 0.3)[i % 4] * 400))
        cells = rng.choice(400, size=k, replace=False)
        owner = rng.randint(0, 4, size=k)
        own = np.zeros((20, 20), dtype=bool)
        occ = np.zeros((20, 20), dtype=bool)
        occ[cells // 20, cells % 20] = True
        mine = cells[owner == 0]
        own[mine // 20, mine % 20] = True
        out.append((own, occ, False, i % 4))
    empty = np.zeros((20, 20), dtype=bool)
    for p in range(4):
        out.append((empty, empty, True, p))
    taken = empty.copy()
    taken[0, 0] = True  # a start corner an opponent sits on
    out.append((empty, taken, True, 0))
    return out


START = ((0, 0), (0, 19), (19, 19), (19, 0))


def _cell_sets(own, occ, first, p):
    """(may_cover, trigger) bool[20,20] from the placement rule on the grid."""
    pad = np.zeros((22, 22), dtype=bool)
    pad[1:21, 1:21] = own
    orth = pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]
    diag = pad[:-2, :-2] | pad[:-2, 2:] | pad[2:, :-2] | pad[2:, 2:]
    may = ~occ & ~orth
    if first:
        trig = np.zeros((20, 20), dtype=bool)
        trig[START[p]] = True
    else:
        trig = diag
    return may, trig & may


def _brute_rows(cells, may, trig):
    """ok word per anchor row 0..19 (bit x = anchor column x)."""
    rows = []
    for r in range(20):
        w = 0
        for x in range(20):
            fit, touch = True, False
            for dr, dc in cells:
                rr, cc = r + dr, x + dc
                if rr > 19 or cc > 19 or not may[rr, cc]:
                    fit = False
                    break
                touch = touch or bool(trig[rr, cc])
            if fit and touch:
                w |= 1 << x
        rows.append(w)
    return rows


def _planes(may, trig):
    """BC / BCP / BCV rows as 64-bit integers: corner rows in the high half, blocked rows
    (with the off-board columns 20..31) in the low half."""
    bc = []
    for r in range(20):
        b = OFFBOARD | sum(1 << c for c in range(20) if not may[r, c])
        c = sum(1 << x for x in range(20) if trig[r, x])
        bc.append(c << 32 | b)
    bcp = [v | v >> 1 for v in bc]
    bcv = [bc[r] | bc[r + 1] if r < 19 else bc[r] for r in range(20)]
    return bc, bcp, bcv


def _scan(planes, h, toks, w1):
    out = []
    for r in range(21 - h):
        b = c = 0
        for k, t in enumerate(toks):
            v = planes[t & 3][r + (t >> 3)]
            if k > 0 and not t & 4:
                v >>= (w1 >> (3 * (k - 1))) & 7
            b |= v & M32
            c |= v >> 32 & M32
        out.append(c & ~b & M32)
    return out


@pytest.fixture(scope="module")
def brute(header):
    _text, _lists, _table, cells, _info = header
    out = []
    for own, occ, first, p in _positions():
        may, trig = _cell_sets(own, occ, first, p)
        out.append((_planes(may, trig), [_brute_rows(cs, may, trig) for cs in cells]))
    assert sum(1 for _pl, rows in out for rws in rows if any(rws)) > 1000  # the positions have moves
    return out


@pytest.mark.parametrize("name", ["BK_CLASS_LIST_ZERO", "BK_CLASS_LIST_COMMON", "BK_CLASS_LIST_PLAIN"])
def test_class_lists_compute_the_rule(header, brute, name):
    _text, lists, table, cells, info = header
    classes = lists[name]
    assert classes[0][0] == 0 and classes[-1][1] == 91
    assert all(a[1] == b[0] for a, b in zip(classes, classes[1:]))  # every entry in one class
    assert sorted(w0 >> 8 for w0, _ in table) == list(range(91))
    for i0, i1, h, toks in classes:
        assert i0 < i1 and 1 <= len(toks) <= 5
        for i in range(i0, i1):
            w0, w1 = table[i]
            g = w0 >> 8
            pid, _n, gh, _gw = info[g]
            assert pid == w0 & 0xFF and gh == h, (name, i)
            for pos, (planes, rows) in enumerate(brute):
                got = _scan(planes, h, toks, w1)
                assert got == rows[g][:21 - h], (name, i, g, pos)
                assert not any(rows[g][21 - h:])


def test_flags_only_on_common_zero_columns(header):
    _text, lists, table, _cells, _info = header
    flagged = {}
    for name in ("BK_CLASS_LIST_ZERO", "BK_CLASS_LIST_COMMON"):
        flagged[name] = 0
        for i0, i1, _h, toks in lists[name]:
            assert not toks[0] & 4  # term 0 is unshifted by position
            for k, t in enumerate(toks):
                if k > 0 and t & 4:
                    flagged[name] += i1 - i0
                    for i in range(i0, i1):
                        assert (table[i][1] >> (3 * (k - 1))) & 7 == 0, (name, i0, k, i)
    assert all(not t & 4 for _a, _b, _h, toks in lists["BK_CLASS_LIST_PLAIN"] for t in toks)
    print("flagged entry-terms:", flagged)
    # no more flags than column-0 terms; merging sub-classes can only lose flags
    zeros = sum(1 for i0, i1, _h, toks in lists["BK_CLASS_LIST_PLAIN"] for i in range(i0, i1)
                for k in range(1, len(toks)) if (table[i][1] >> (3 * (k - 1))) & 7 == 0)
    assert zeros >= flagged["BK_CLASS_LIST_ZERO"] >= flagged["BK_CLASS_LIST_COMMON"]


def test_header_is_the_generators_output(header, monkeypatch):
    monkeypatch.delenv("BK_GEN_ZERO", raising=False)
    monkeypatch.delenv("BK_GEN_VPAIR", raising=False)
    spec = importlib.util.spec_from_file_location("gen_tables", os.path.join(ROOT, "tools", "gen_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = header[0]
    table = gen.orientations()
    if sys.version_info[:2] == (3, 10):
        assert gen.render(table) == text
    else:  # the cell-hash section restates CPython 3.10's tuple hash
        monkeypatch.setattr(gen, "render_cell_hash", lambda: [])
        want = gen.render(table)
        assert text.startswith(want[:-1])
