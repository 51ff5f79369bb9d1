"""tools/kernel_isa_diff.py --rename on two hand-written listing snippets (tests/golden/isa_rename):
a kernel whose symbol changed and whose instructions did not, one whose instructions changed too,
and one that kept its name."""
from __future__ import annotations

import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = os.path.join(REPO, "tests", "golden", "isa_rename", "old.s.txt")
NEW = os.path.join(REPO, "tests", "golden", "isa_rename", "new.s.txt")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location(
        "kernel_isa_diff", os.path.join(REPO, "tools", "kernel_isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tool, capsys, *args):
    status = tool.main([OLD, NEW, *args])
    return status, capsys.readouterr().out.splitlines()


def test_without_rename_a_changed_symbol_is_missing_on_both_sides(tool, capsys):
    status, out = _run(tool, capsys, ".")
    assert status == 1
    assert out == ["missing in new  k_grew_dual", "missing in old  k_grew_rule1",
                   "identical       2      2  k_kept",
                   "missing in new  k_twin_dual", "missing in old  k_twin_rule1",
                   "1 of 5 kernels identical"]


def test_renamed_identical_pair(tool, capsys):
    """The function number in the local labels differs between the two sides; nothing else does."""
    status, out = _run(tool, capsys, "k_twin|k_kept", "--rename", "_dual$=_rule1")
    assert status == 0
    assert out == ["identical       2      2  k_kept", "identical       6      6  k_twin_rule1",
                   "2 of 2 kernels identical"]


def test_renamed_different_pair(tool, capsys):
    status, out = _run(tool, capsys, ".", "--rename", "k_grew_dual=k_grew_rule1",
                       "--rename", "^k_twin_dual$=k_twin_rule1", "--show", "20")
    assert status == 1
    assert out[0] == "different       3      4  k_grew_rule1"
    assert "    +s_nop 0" in out
    assert out[-3:] == ["identical       2      2  k_kept", "identical       6      6  k_twin_rule1",
                        "2 of 3 kernels identical"]
    assert not any(line.startswith("missing") for line in out)


def test_renames_apply_in_order_and_a_bad_one_is_refused(tool, capsys):
    status, out = _run(tool, capsys, "k_twin", "--rename", "_dual$=_x", "--rename", "_x$=_rule1")
    assert (status, out[-1]) == (0, "1 of 1 kernels identical")
    with pytest.raises(SystemExit):
        tool.main([OLD, NEW, ".", "--rename", "no-equals-sign"])
