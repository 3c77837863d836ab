"""Per-column residual bins of bamd_column_hist without a GPU: the header states the n_ed < 0 domain, and the ABI did not grow."""
import os
import re

from baler_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "baler_amd.h")) as f:
        return f.read()


def test_header_states_the_per_column_domain():
    src = _header()
    text = src[src.index("Replaces: the four np.histogram calls per column"):src.index("int bamd_column_hist(")]
    flat = " ".join(text.replace("*", " ").split())
    assert "n_ed < 0: per-column residual bins" in flat
    assert "edges_resid is then (n_cols, -n_ed) float64, one strictly increasing edge array per column" in flat
    assert "counts_resid is (n_cols, -n_ed - 1)" in flat
    assert "-n_ed is 2 .. 1025 (n_ed = -1 and n_ed < -1025: BAMD_ERR_INVALID)" in flat
    assert "the first edge may be -inf and the last +inf" in flat
    assert "n_er and n_ev keep their meaning" in flat


def test_no_new_export_and_no_changed_signature():
    src = _header()
    assert "#define BAMD_ABI_VERSION 1" in src
    assert len(native.SYMBOLS) == 38 == len(set(native.SYMBOLS))
    decl = src[src.index("int bamd_column_hist("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int bamd_column_hist(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col, "
                    "double cut, const double *edges_resp, int n_er, int64_t *counts_resp, const double *edges_resid, int n_ed, "
                    "int64_t *counts_resid, const double *edges_val, int n_ev, int64_t *counts_before, int64_t *counts_after, "
                    "int accumulate, void *stream)")
    with open(os.path.join(REPO, "baler_amd", "csrc", "colstats.hip")) as f:
        hip = f.read()
    exported = re.findall(r"^int (bamd_\w+)\(", hip[hip.index('extern "C"'):], flags=re.M)
    assert exported == ["bamd_column_moments", "bamd_column_hist"]
