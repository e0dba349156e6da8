"""The step log's records against include/blokus_hip.h: struct sizes and field offsets of
bk_step and bk_step_rec equal the numpy dtypes', the status bits and the new symbols are
the binding's.  No GPU."""
import os
import re

from reinforcementlearning_blokus_amd import _native as N
from tests.conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "blokus_hip.h")).read()
CTYPE_SIZE = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4}


def struct_layout(name):
    """[(field, offset, bytes)] of a header struct made of fixed-width unsigned fields, laid out
    with natural alignment, and its size."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for ctype, decls in re.findall(r"(uint\d+_t)\s+([^;]+);", body):
        size = CTYPE_SIZE[ctype]
        for decl in decls.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", decl)
            count = int(m.group(2) or 1)
            assert off % size == 0, f"{name}.{m.group(1)} would be padded"
            fields.append((m.group(1), off, size * count))
            off += size * count
    return fields, off


def check(name, dtype):
    fields, size = struct_layout(name)
    assert size == dtype.itemsize and [f for f, _, _ in fields] == list(dtype.names)
    for f, off, nbytes in fields:
        assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == nbytes, f


def test_step_record_layout():
    check("bk_step_rec", N.STEP_REC_DTYPE)
    assert N.STEP_REC_DTYPE.itemsize == 64 and N.STEP_REC_DTYPE.itemsize % 8 == 0
    assert N.load().bk_step_rec_size() == N.STEP_REC_DTYPE.itemsize


def test_step_layout():
    check("bk_step", N.STEP_DTYPE)
    assert N.STEP_DTYPE.itemsize == 8


def test_status_bits_and_symbols():
    bits = dict(re.findall(r"#define BK_STEP_ST_(\w+)\s+(\d+)u", HEADER))
    assert {k: int(v) for k, v in bits.items()} == {"TABLE": N.STEP_ST_TABLE, "STATE": N.STEP_ST_STATE,
                                                    "MOVE": N.STEP_ST_MOVE}
    assert (N.STEP_ST_TABLE, N.STEP_ST_STATE) == (N.SNAP_ST_TABLE, N.SNAP_ST_STATE)
    assert "bk_step_metrics" in N.EXPORTS and "bk_step_rec_size" in N.EXPORTS
    lib = N.load()
    assert hasattr(lib, "bk_step_metrics") and hasattr(lib, "bk_step_rec_size")
    assert lib.bk_step_metrics(None, None, None, None, None, None, 0, None, N.MEM_HOST) == N.EINVAL  # no GPU call
