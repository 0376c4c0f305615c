"""The host model loader pinned table by table: every scalar and every table that csrc/myo_host.h derives from a model blob, read back
through myo_model_size / myo_model_table, against tests/golden/host_tables.json (tests/host_table_cases.py: the models, the names and
what the fixture keeps).  The fixture was written by the loader as it was before it was cut into stages; the kernels read these
tables and nothing else of a model, so a loader that reproduces them bit for bit leaves every trajectory where it was.

A table's bytes are compared by their sha256.  To see WHERE a table differs, write the values of a known-good checkout to a file
(`python tools/make_golden.py host_tables --values good.npz` there) and name it in MYO_HOST_TABLES_VALUES: the failure then gives the
first differing index of every table that differs."""
import json
import os

import numpy as np
import pytest

import host_table_cases as htc


@pytest.fixture(scope="module")
def golden():
    return json.load(open(htc.FIXTURE))


def first_difference(case, name, got):
    path = os.environ.get("MYO_HOST_TABLES_VALUES")
    if not path:
        return "(set MYO_HOST_TABLES_VALUES to a values file of a good checkout for the first differing index)"
    want = np.load(path)["%s/%s" % (case, name)]
    if want.shape != got.shape:
        return "%d elements, the good checkout has %d" % (got.size, want.size)
    bad = np.nonzero(want.view(np.uint8).reshape(want.size, -1) != got.view(np.uint8).reshape(got.size, -1))[0]
    return "first difference at [%d]: %r, the good checkout has %r" % (bad[0], got[bad[0]], want[bad[0]]) if bad.size else "same values as the good checkout"


def test_fixture_covers_the_cases_and_every_table(golden):
    assert sorted(golden) == sorted(htc.case_names())
    for case, g in golden.items():
        assert sorted(g["tables"]) == sorted(htc.table_names()), case
        assert sorted(g["int"]) == sorted(htc.INT_SCALARS) and sorted(g["real"]) == sorted(n for n, _ in htc.REAL_SCALARS), case


@pytest.mark.parametrize("case", htc.case_names())
def test_loader_reproduces_the_pinned_tables(case, golden, emu_lib):
    want = golden[case]
    read = htc.read_model(htc.load_case(case, emu_lib))
    got = htc.digest(read)
    wrong = ["%s = %r, pinned %r" % (n, got["int"][n], v) for n, v in want["int"].items() if got["int"][n] != v]
    wrong += ["%s = %r, pinned %r" % (n, got["real"][n], v) for n, v in want["real"].items() if got["real"][n] != v]
    if got["arrow_pad"] != want["arrow_pad"]:
        wrong.append("arrow_pad = %#x, pinned %#x" % (got["arrow_pad"], want["arrow_pad"]))
    for n, w in want["tables"].items():
        if got["tables"][n] != w:
            wrong.append("table %s: %s, pinned %s; %s" % (n, got["tables"][n], w, first_difference(case, n, read["tables"][n])))
    assert not wrong, "%s: %d differences\n" % (case, len(wrong)) + "\n".join(wrong)
