"""Every entry of lap/_hip.py:SIGNATURES is declared in include/lapwarm_hip.h with that many parameters and exported
by the library.  The C ABI keeps its workspace sizes, its argument checks and their order (abi_contract_common.py against
tests/golden/abi_contract.json), and every too-small workspace is reported in lapwarm_last_error().  No GPU: every
recorded call returns before its first HIP call."""
import ctypes as ct
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

import abi_contract_common as acc
from conftest import ROOT
from host_common import lib  # noqa: F401
from lap import _hip

GOLDEN = Path(__file__).resolve().parent / "golden" / "abi_contract.json"
HEADER = (ROOT / "include" / "lapwarm_hip.h").read_text()
# entries whose bound types are asserted in full, not only counted
_VP, _INT = _hip.c_vp, ct.c_int
EXACT_SIGNATURES = {
    "lapwarm_ragged_duals_workspace_bytes": (ct.c_size_t, [_INT, _INT]),
    "lapwarm_oracle_duals_ragged_workspace_bytes": (ct.c_size_t, [_INT, _INT]),
    # host_sizes (3) is a host array; ld, batch, N; ws_bytes (14); every other argument a device or stream pointer
    "lapwarm_oracle_duals_ragged": (_INT, [_VP] * 3 + [_hip.c_ip] + [_INT] * 3 + [_VP] * 7 + [ct.c_size_t, _VP]),
}


@pytest.mark.parametrize("name", sorted(_hip.SIGNATURES))
def test_header_declares_and_library_exports_the_entry_with_its_argument_count(lib, name):
    """Every entry the binding lists: declared in the header with as many parameters as the binding has argument
    types, and exported by the library."""
    res, args = _hip.SIGNATURES[name]
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, HEADER)
    assert m, f"{name} is not declared in lapwarm_hip.h"
    params = m.group(1).strip()
    declared = 0 if params in ("", "void") else len(params.split(","))
    assert declared == len(args), (name, m.group(1))
    assert hasattr(lib, name), name
    if name in EXACT_SIGNATURES:
        assert (res, args) == EXACT_SIGNATURES[name], name


@pytest.fixture(scope="module")
def contract():
    """One record from a fresh interpreter with the library's tuning variables cleared: it reads them once."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("LAPWARM_")}
    r = subprocess.run([sys.executable, acc.__file__], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout), json.loads(GOLDEN.read_text())


def test_workspace_sizes_are_unchanged(contract):
    got, want = contract
    assert set(got["sizes"]) == set(want["sizes"])
    for name, values in want["sizes"].items():
        assert got["sizes"][name] == values, name
    points = (len(acc.GRID_BATCH) + 2) * (len(acc.GRID_N) + 2)
    assert all(len(want["sizes"][name]) == points for name in acc.TWO_INT_SIZES)
    assert any(want["sizes"]["seeded"]) and 0 in want["sizes"]["seeded"]  # in range and out of range are both there


def test_return_codes_and_check_order_are_unchanged(contract):
    got, want = contract
    assert set(got["codes"]) == set(want["codes"])
    for symbol, cases in want["codes"].items():
        assert got["codes"][symbol] == cases, symbol
        assert all(code > -1000 for code in cases.values()), symbol  # nothing recorded reached the HIP runtime
    seen = {code for cases in want["codes"].values() for code in cases.values()}
    assert seen == {0, -1, -2, -4, -5, -6}


def test_a_short_workspace_sets_the_error_text(contract):
    got, want = contract
    short = {symbol for symbol, cases in want["codes"].items() if cases.get("ws short") == -1}
    assert set(got["short_text"]) == short and len(short) == 29
    for symbol, text in got["short_text"].items():
        assert text.startswith("workspace too small"), (symbol, text)
