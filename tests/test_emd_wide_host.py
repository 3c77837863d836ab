"""bamd_emd_rows on wide tables, the parts a machine without a GPU can check: the reference fixture against oracle/c_oracle (the
reference every GPU test of tests/test_gpu_emd_wide.py compares with), and the public surface."""
import os
import re

import emd_wide_cases as cases
from baler_amd import native
from oracle import c_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_g22_emd_wide_oracle(golden):
    g = golden("g22_emd_wide.npz")
    assert sorted(str(n) for n in g["names"]) == sorted(cases.CASES)
    for name, x, recon, want in cases.fixture_tables(g):
        got = orc.emd_rows(x, recon)
        print(f"g22 {name} {x.shape}: oracle rel {abs(got - want) / abs(want):.3e}")
        assert abs(got - want) < 1e-12 * abs(want), name


def test_fixture_holds_no_tables(golden):
    g = golden("g22_emd_wide.npz")
    assert set(g.files) == {"names", "shapes_seeds", "emd"}
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g22_emd_wide.npz")) < 2048


def test_header_states_the_wide_contract():
    text = open(os.path.join(REPO, "include", "baler_amd.h")).read()
    doc = text[text.index("Replaces: the EMD term"):text.index("int bamd_emd_rows(")]
    assert "<= 64" not in doc
    assert "n_cols <= 4096" in doc and "NaN" in doc and "inf" in doc
    assert re.search(r"grid|workgroups", doc), "the comment says that the result does not depend on the grid"


def test_symbol_count_unchanged():
    assert len(native.SYMBOLS) == 38 and "bamd_emd_rows" in native.SYMBOLS
