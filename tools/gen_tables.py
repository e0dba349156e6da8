#!/usr/bin/env python3
"""Emit reinforcementlearning_blokus_amd/csrc/orient_table.h.

Restates engine/pieces.py:147-253 (generate_orientations_for_piece) for the 21
shapes of engine/pieces.py:289-356: variants rot0..rot270 (numpy.rot90, counter-
clockwise), then fliplr and its three rotations; a variant whose sorted normalized
offsets were already seen is dropped.  The global orientation id g runs piece-major
(piece 1 first), orientation index ascending: g order == reference list order.

tests/test_stencil_table.py checks the committed header against this output and its
stencil class lists against the placement rule; tests/test_stencil_mux_table.py does the
same for the per-phase lists (`--mux-stats` prints their static op counts).
"""
import os

SHAPES = [
    "1", "11", "111", "10|11", "1111", "11|11", "111|010", "10|10|11", "011|110", "110|011",
    "011|110|010", "11111", "10|10|10|11", "10|11|01|01", "11|11|10", "111|010|010", "101|111",
    "100|100|111", "100|110|011", "010|111|010", "10|11|10|10",
]


def rot90(m):
    h, w = len(m), len(m[0])
    return [[m[j][w - 1 - i] for j in range(h)] for i in range(w)]


def fliplr(m):
    return [row[::-1] for row in m]


def orientations():
    table = []
    for pid, s in enumerate(SHAPES, start=1):
        base = [[int(ch) for ch in row] for row in s.split("|")]
        variants = [base]
        for _ in range(3):
            variants.append(rot90(variants[-1]))
        variants.append(fliplr(base))
        for _ in range(3):
            variants.append(rot90(variants[-1]))
        seen = []
        for v in variants:
            cells = sorted((r, c) for r, row in enumerate(v) for c, x in enumerate(row) if x)
            if cells in seen:
                continue
            seen.append(cells)
            table.append((pid, len(seen) - 1, cells, len(v), len(v[0])))
    return table


# stencil term kinds: one cell, a horizontal pair (plane BP = B | B >> 1), a vertical
# pair (plane BV[R] = B[R] | B[R + 1])
KINDS = {"s": 0, "p": 1, "v": 2}
VPAIR = os.environ.get("BK_GEN_VPAIR", "0") == "1"  # measured: 2 waves/SIMD needed, net slower


def _placements(cells):
    cs = set(cells)
    out = []
    for (r, c) in cells:
        out.append(("s", r, c, frozenset([(r, c)])))
        if (r, c + 1) in cs:
            out.append(("p", r, c, frozenset([(r, c), (r, c + 1)])))
        if VPAIR and (r + 1, c) in cs:
            out.append(("v", r, c, frozenset([(r, c), (r + 1, c)])))
    return out


def stencil_terms(cells):
    """Cover an orientation's cells with the fewest singles / horizontal / vertical pairs (overlap
    allowed: the stencil ORs shifted rows, so covering a cell twice is harmless).
    Returns [(kind, d, c), ...] with a column-0 term first (it needs no shift), the
    rest sorted by (d, kind, c)."""
    import itertools
    target = frozenset(cells)
    P = _placements(cells)
    for k in range(1, 6):
        for combo in itertools.combinations(P, k):
            if frozenset().union(*[x[3] for x in combo]) == target:
                terms = sorted(((x[0], x[1], x[2]) for x in combo), key=lambda t: (t[1], t[0], t[2]))
                z = next(i for i, t in enumerate(terms) if t[2] == 0)
                return [terms[z]] + terms[:z] + terms[z + 1:]
    raise AssertionError(cells)


# Zero-column flags.  A term at column 0 of its orientation needs no shift; term 0 is
# one by position, any later one can carry a flag in its class token so the stencil
# reads the plane row directly.  Per class of the plain list (its index there):
#   "keep"   no flag: the class's code is the unflagged one
#   "common" flag the terms whose column is 0 in every entry of the class
#   "split"  one sub-class per zero pattern of its entries, every zero flagged
# ZERO_MODES is the one list a sweep edits (`--zero-stats` prints each class's weighted
# shift counts).  BK_GEN_ZERO overrides it for one regeneration: a mode name (every
# class), or "mode:ci,ci;mode:ci" (the rest keep).  Measured: every zero
# shift removed -- split where the entries' zero patterns differ, common where they
# agree -- 46.3 M frontier-order playouts/s against 44.6 M with common flags only and
# 43.1 M with none; the classes not listed have no column-0 term after term 0.
ZERO_DEFAULT = "keep"
ZERO_MODES = {
    **{ci: "common" for ci in (5, 6, 13, 14, 21, 22, 23, 24, 36, 40, 41, 48)},
    **{ci: "split" for ci in (7, 8, 11, 12, 15, 16, 25, 26, 27, 28, 29, 30, 31, 32, 35, 37, 38, 42, 43, 44, 45, 46)},
}


def _zero_modes():
    env = os.environ.get("BK_GEN_ZERO")
    if env is None:
        return ZERO_MODES, ZERO_DEFAULT
    if ":" not in env:
        return {}, env
    modes = {}
    for part in env.split(";"):
        mode, _, ids = part.partition(":")
        modes.update({int(ci): mode for ci in ids.split(",") if ci})
    return modes, "keep"


def zero_mode(ci):
    modes, default = _zero_modes()
    m = modes.get(ci, default)
    assert m in ("keep", "common", "split"), m
    return m


def plain_classes(table):
    """{(height, ((d, kind), ...)): [(g, piece, (c0, c1, ...)), ...]} and the keys in list order."""
    classes = {}
    for g, (pid, _o, cells, h, _w) in enumerate(table):
        terms = stencil_terms(cells)
        key = (h, tuple((d, KINDS[k]) for k, d, _c in terms))
        classes.setdefault(key, []).append((g, pid, tuple(c for _k, _d, c in terms)))
    order = sorted(classes, key=lambda k: (k[0], len(k[1]), tuple(d * 4 + kd for d, kd in k[1])))
    return classes, order


def zero_classes(table):
    """The flagged class list: [(height, ((d, kind, zero), ...), entries)] in table order.
    Sub-classes of a split class stay adjacent, so a plain class is a contiguous range of
    the same table."""
    classes, order = plain_classes(table)
    out = []
    for ci, key in enumerate(order):
        h, terms = key
        ents = classes[key]
        mode = zero_mode(ci)
        if mode == "split":
            pats = sorted({tuple(int(j > 0 and c == 0) for j, c in enumerate(e[2])) for e in ents})
            groups = [(p, [e for e in ents if tuple(int(j > 0 and c == 0) for j, c in enumerate(e[2])) == p])
                      for p in pats]
        elif mode == "common":
            groups = [(tuple(int(j > 0 and all(e[2][j] == 0 for e in ents)) for j in range(len(terms))), ents)]
        else:
            groups = [((0,) * len(terms), ents)]
        for pat, es in groups:
            out.append((h, tuple((d, kd, z) for (d, kd), z in zip(terms, pat)), es))
    return out


def _render_list(name, cls):
    lines = [f"#define {name}(X) \\"]
    i = 0
    for h, terms, ents in cls:
        toks = ", ".join(str(d * 8 + 4 * z + kd) for d, kd, z in terms)
        lines.append(f"    X({i}, {i + len(ents)}, {h}, {toks}) \\")
        i += len(ents)
    lines.append("")
    return lines


def render_classes(table):
    """Stencil classes.  A class = (height, term sequence [(d, kind, zero)]) -- the static
    shape of the straight-line code that scans it; the column shifts of the unflagged
    terms 1.. are per-orientation (uniform) operands.  Per orientation 2 words in class
    order: w0 = piece_id | g << 8, w1 = column of term k (k >= 1) at bits 3(k-1).
    BK_CLASS_LIST_ZERO(X) expands X(i0, i1, height, t0, t1, ...) per class with
    t = d * 8 + 4 * zero + kind (KINDS); zero = the column is 0 in every entry of the class
    and the term is not shifted (ZERO_MODES).  Two more lists index the same table with
    every split undone: BK_CLASS_LIST_COMMON keeps the flags all sub-classes share (for
    a unit that pays per class, such as the lane-pair scan), BK_CLASS_LIST_PLAIN has no
    flag: the code of a unit that ignores them."""
    cls = zero_classes(table)

    def merged(keep_flags):  # sub-classes merged back; a flag stays where all of them have it
        out = []
        for h, terms, ents in cls:
            if out and out[-1][0] == h and [t[:2] for t in out[-1][1]] == [t[:2] for t in terms]:
                pt = tuple((d, kd, z and z2) for (d, kd, z), (_d, _k, z2) in zip(out[-1][1], terms))
                out[-1] = (h, pt, out[-1][2] + ents)
            else:
                out.append((h, terms, list(ents)))
        return [(h, tuple((d, kd, z if keep_flags else 0) for d, kd, z in t), e) for h, t, e in out]

    lines = [f"#define BK_NUM_CLASSES {len(cls)}",
             f"#define BK_STENCIL_TERMS {sum(len(t) * len(e) for _h, t, e in cls)}"]
    lines += _render_list("BK_CLASS_LIST_ZERO", cls)
    lines += _render_list("BK_CLASS_LIST_COMMON", merged(True))
    lines += _render_list("BK_CLASS_LIST_PLAIN", merged(False))
    lines.append("#define BK_CLASS_TABLE_INIT { \\")
    for _h, _t, ents in cls:
        for g, pid, cols in ents:
            w1 = sum(c << (3 * (j - 1)) for j, c in enumerate(cols) if j > 0)
            lines.append(f"    {{{hex(pid | (g << 8))}, {hex(w1)}}}, \\")
    lines.append("}")
    return lines


# Per-phase second planes (-DBK_STENCIL_MUX).  The class loop is straight-line code and
# the order of the orientations is free, so the 20 rows of the second plane can be
# rebuilt between groups of classes; each orientation is scanned in the phase whose
# plane covers it most cheaply.  A phase's kind-1 term is one placement of its shape:
#   p  horizontal pair    B | B >> 1             (the plane of the lists above)
#   t  horizontal triple  B | B >> 1 | B >> 2
#   u  vertical triple    B[R] | B[R + 1] | B[R + 2]
#   q  2 x 2 square       p[R] | p[R + 1]
MUX_SHAPES = {"p": ((0, 0), (0, 1)), "t": ((0, 0), (0, 1), (0, 2)), "u": ((0, 0), (1, 0), (2, 0)),
              "q": ((0, 0), (0, 1), (1, 0), (1, 1))}
# MUX_PHASES is the order in which a tie between phases is settled (the earlier one); the
# kernel scans q right after p, whose rows it is made of.  BK_GEN_MUX overrides the phases
# for one regeneration ("p,t,u": the pass without q, for an A/B).
MUX_PHASES = tuple(os.environ.get("BK_GEN_MUX", "p,t,u,q").split(","))
MUX_MAX_COL = 3  # a shift of <= 3 moves C bits only into B's off-board bits; w1 keeps 3 bits per term


def mux_covers(cells, shape):
    """The cheapest covers of an orientation by single cells and placements of one extra
    shape, every term at a column <= MUX_MAX_COL and one of them at column 0.  Cost per
    anchor row: one OR-type op per term and one shift per term at a non-zero column;
    ties go to fewer terms.  Returns (cost, [terms, ...]): every cover of that cost and
    length, each as [(kind, d, c)] in class order (a column-0 term first, the rest by
    (d, kind, c)) and once per choice of the first term; kind 1 = the shape.  None where
    the rules leave no cover (the horizontal I5 with singles and u)."""
    import itertools
    cs = set(cells)
    target = frozenset(cells)
    P = [(0, r, c, frozenset([(r, c)])) for r, c in cells if c <= MUX_MAX_COL]
    for r, c in cells:
        sub = frozenset((r + dr, c + dc) for dr, dc in MUX_SHAPES[shape])
        if c <= MUX_MAX_COL and sub <= cs:
            P.append((1, r, c, sub))
    best, covers = None, []
    for k in range(1, 6):
        for combo in itertools.combinations(P, k):
            if frozenset().union(*[x[3] for x in combo]) != target or all(x[2] for x in combo):
                continue
            terms = sorted(((x[0], x[1], x[2]) for x in combo), key=lambda t: (t[1], t[0], t[2]))
            rank = (k + sum(1 for t in terms if t[2]), k)
            if best is None or rank < best:
                best, covers = rank, []
            if rank == best:
                covers += [[terms[z]] + terms[:z] + terms[z + 1:] for z, t in enumerate(terms) if t[2] == 0]
    return (best[0], covers) if covers else None


def mux_assign(table, phases=MUX_PHASES):
    """[(phase, cost, covers)] per orientation: the phase with its cheapest cover; ties go
    to fewer terms, then to the earlier phase."""
    out = []
    for _pid, _o, cells, _h, _w in table:
        cands = []
        for pi, ph in enumerate(phases):
            cov = mux_covers(cells, ph)
            if cov is not None:
                cands.append((cov[0], len(cov[1][0]), pi, ph, cov[1]))
        cost, _nt, _pi, ph, covers = min(cands)
        out.append((ph, cost, covers))
    return out


def mux_classes(table, phases=MUX_PHASES):
    """{phase: [(height, ((d, kind, zero), ...), entries)]}, entries as in zero_classes.
    A class is keyed by its zero pattern too, so every column-0 term is flagged.  Where an
    orientation has several covers of its cheapest cost, the one that shares a class with
    the most others is taken (greedily, the largest class first): fewer classes, less code."""
    assign = mux_assign(table, phases)
    out = {}
    for ph in phases:
        cands = {}  # class key -> {g: columns}
        for g, ((_pid, _o, _cells, h, _w), (aph, _cost, covers)) in enumerate(zip(table, assign)):
            if aph != ph:
                continue
            for terms in covers:
                key = (h, tuple((d, k, int(j > 0 and c == 0)) for j, (k, d, c) in enumerate(terms)))
                cands.setdefault(key, {}).setdefault(g, tuple(c for _k, _d, c in terms))
        classes, left = {}, {g for m in cands.values() for g in m}
        while left:
            key = min(cands, key=lambda k: (-len(left & set(cands[k])), k))
            classes[key] = [(g, table[g][0], cands[key][g]) for g in sorted(left & set(cands[key]))]
            left -= set(cands[key])
        order = sorted(classes, key=lambda k: (k[0], len(k[1]), tuple(d * 4 + kd for d, kd, _z in k[1]),
                                               tuple(z for _d, _kd, z in k[1])))
        out[ph] = [(h, terms, classes[(h, terms)]) for h, terms in order]
    return out


def mux_stats(table, phases=MUX_PHASES):
    """Per phase: (phase, orientations, plain classes, classes, weighted NT, weighted nz);
    the weight is the anchor rows 21 - h."""
    rows = []
    for ph, cls in mux_classes(table, phases).items():
        nt = sum((21 - h) * len(t) * len(e) for h, t, e in cls)
        nz = sum((21 - h) * sum(1 for c in cols if c) for h, _t, e in cls for _g, _pid, cols in e)
        plain = {(h, tuple(x[:2] for x in t)) for h, t, _e in cls}
        rows.append((ph, sum(len(e) for _h, _t, e in cls), len(plain), len(cls), nt, nz))
    return rows


def render_mux(table):
    """The per-phase lists of -DBK_STENCIL_MUX: BK_CLASS_LIST_MUX_P / _T / _U / _Q in the token
    format of the lists above (kind 1 = the second plane of the phase), indexing a table
    of their own (the term columns differ), phase after phase."""
    cls = mux_classes(table)
    lines = [f"#define BK_NUM_CLASSES_MUX {sum(len(c) for c in cls.values())}"]
    i = 0
    for ph in MUX_PHASES:
        lines.append(f"#define BK_CLASS_LIST_MUX_{ph.upper()}(X) \\")
        for h, terms, ents in cls[ph]:
            toks = ", ".join(str(d * 8 + 4 * z + kd) for d, kd, z in terms)
            lines.append(f"    X({i}, {i + len(ents)}, {h}, {toks}) \\")
            i += len(ents)
        lines.append("")
    lines.append("#define BK_CLASS_TABLE_MUX_INIT { \\")
    for ph in MUX_PHASES:
        for _h, _t, ents in cls[ph]:
            for g, pid, cols in ents:
                w1 = sum(c << (3 * (j - 1)) for j, c in enumerate(cols) if j > 0)
                lines.append(f"    {{{hex(pid | (g << 8))}, {hex(w1)}}}, \\")
    lines.append("}")
    return lines


def zero_stats(table):
    """Per plain class: anchor-row-weighted shifts, zero shifts, and the zero shifts a
    'common' flagging removes (a sweep's ranking)."""
    classes, order = plain_classes(table)
    rows = []
    for ci, key in enumerate(order):
        h, terms = key
        ents = classes[key]
        nr = 21 - h
        shifts = nr * (len(terms) - 1) * len(ents)
        zeros = nr * sum(1 for e in ents for j, c in enumerate(e[2]) if j > 0 and c == 0)
        common = nr * len(ents) * sum(1 for j in range(1, len(terms)) if all(e[2][j] == 0 for e in ents))
        rows.append((ci, h, len(terms), len(ents), shifts, zeros, common, zero_mode(ci)))
    return rows


def render_cell_hash():
    """hash((r, c)) of this CPython (3.10: xxHash-based tuplehash over the int hashes),
    as the 64-bit pattern: the frontier sets' slot order depends on it
    (engine/board.py:70 player_frontiers are sets of (row, col) tuples)."""
    import sys
    assert sys.version_info[:2] == (3, 10), "the reference runs CPython 3.10"
    vals = [hash((r, c)) & (2**64 - 1) for r in range(20) for c in range(20)]
    lines = ["// CPython 3.10 hash((r, c)) for cell r*20+c (frontier set slot order)",
             "#define BK_CELL_HASH_INIT { \\"]
    for i in range(0, 400, 4):
        lines.append("    " + ", ".join(f"{v:#018x}ull" for v in vals[i:i + 4]) + ", \\")
    lines.append("}")
    return lines


def render(table):
    lines = [
        "// Generated by tools/gen_tables.py -- do not edit.",
        "// 91 orientations of the 21 reference pieces (engine/pieces.py:147-356),",
        "// global id g piece-major / orientation-ascending == reference list order.",
        "#pragma once",
        "#include <stdint.h>",
        f"#define BK_NUM_ORIENTS {len(table)}",
        "// info: piece_id | ncells << 8 | height << 16 | width << 24",
        "static const uint32_t kOrientInfoHost[BK_NUM_ORIENTS] = {",
    ]
    for pid, _o, cells, h, w in table:
        lines.append(f"    {pid} | ({len(cells)} << 8) | ({h} << 16) | ({w} << 24),")
    lines.append("};")
    lines.append("// cells: row << 8 | col, sorted (row-major); unused entries 0")
    lines.append("static const uint32_t kOrientCellsHost[BK_NUM_ORIENTS][5] = {")
    for _pid, _o, cells, _h, _w in table:
        vals = [f"({r} << 8) | {c}" for r, c in cells] + ["0"] * (5 - len(cells))
        lines.append("    {" + ", ".join(vals) + "},")
    lines.append("};")
    lines.append("// orientation index within the piece (Move.orientation)")
    lines.append("static const uint8_t kOrientIndexHost[BK_NUM_ORIENTS] = {")
    lines.append("    " + ", ".join(str(o) for _p, o, _c, _h, _w in table))
    lines.append("};")
    lines.append("// initializer lists for __constant__ device copies")
    lines.append("#define BK_ORIENT_INFO_INIT { \\")
    for pid, _o, cells, h, w in table:
        lines.append(f"    {pid} | ({len(cells)} << 8) | ({h} << 16) | ({w} << 24), \\")
    lines.append("}")
    lines.append("#define BK_ORIENT_CELLS_INIT { \\")
    for _pid, _o, cells, _h, _w in table:
        vals = [f"({r} << 8) | {c}" for r, c in cells] + ["0"] * (5 - len(cells))
        lines.append("    {" + ", ".join(vals) + "}, \\")
    lines.append("}")
    lines.append("// rows: per orientation and piece row d (0..4): ncells << 16 | col_j << 3j")
    lines.append("#define BK_ORIENT_ROWS_INIT { \\")
    for _pid, _o, cells, _h, _w in table:
        words = []
        for d in range(5):
            cols = [c for r, c in cells if r == d]
            w = (len(cols) << 16) | sum(c << (3 * j) for j, c in enumerate(cols))
            words.append(hex(w))
        lines.append("    {" + ", ".join(words) + "}, \\")
    lines.append("}")
    lines += render_classes(table)
    lines += render_mux(table)
    lines += render_cell_hash()
    return "\n".join(lines) + "\n"


def main():
    import sys
    if "--zero-stats" in sys.argv:
        print("class  H  terms entries  shifts  zero  common  mode")
        tot = [0, 0, 0]
        for ci, h, nt, ne, sh, z, cm, mode in zero_stats(orientations()):
            print(f"{ci:5d} {h:2d} {nt:6d} {ne:7d} {sh:7d} {z:5d} {cm:7d}  {mode}")
            tot = [tot[0] + sh, tot[1] + z, tot[2] + cm]
        print("total", *tot)
        return
    if "--mux-stats" in sys.argv:
        table = orientations()
        for phases in (("p",), ("p", "t"), ("p", "t", "u"), ("p", "t", "u", "q")):
            print("phases", " ".join(phases))
            print("  phase orients plain classes    NT    nz")
            tot = [0, 0]
            for ph, no, npl, nc, nt, nz in mux_stats(table, phases):
                print(f"  {ph:>5} {no:7d} {npl:5d} {nc:7d} {nt:5d} {nz:5d}")
                tot = [tot[0] + nt, tot[1] + nz]
            print(f"  total NT {tot[0]} nz {tot[1]} NT+nz {sum(tot)}")
        return
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                       "reinforcementlearning_blokus_amd", "csrc", "orient_table.h")
    with open(out, "w") as f:
        f.write(render(orientations()))
    print("wrote", os.path.normpath(out))


if __name__ == "__main__":
    main()
