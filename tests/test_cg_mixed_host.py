"""The mixed-precision CG's entry points exist and refuse a null context (no GPU needed)."""
import ctypes

import pytest

sm = pytest.importorskip("schwingermodel_amd")
lib = sm.lib


def test_symbols_exist():
    assert hasattr(lib, "sm_cg_precision") and hasattr(lib, "sm_cg_mixed_last")


def test_null_context_is_an_argument_error():
    mode = ctypes.c_int(-7)
    assert lib.sm_cg_precision(None, 1, ctypes.byref(mode)) == 1  # SM_ERR_ARG
    assert mode.value == -7
    assert lib.sm_cg_precision(None, 1, None) == 1
    info = sm.CGMixedInfo()
    assert lib.sm_cg_mixed_last(None, ctypes.byref(info)) == 1
    assert lib.sm_cg_mixed_last(None, None) == 1


def test_info_struct_matches_header(tmp_path):
    """The ctypes mirror of sm_cg_mixed_info has the header's size and offsets."""
    import os
    import subprocess
    from conftest import REPO
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sm_hip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(sm_cg_mixed_info));']
    for fname, _ in sm.CGMixedInfo._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(sm_cg_mixed_info, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln}
    assert got["size"] == ctypes.sizeof(sm.CGMixedInfo)
    for fname, _ in sm.CGMixedInfo._fields_:
        assert got[fname] == getattr(sm.CGMixedInfo, fname).offset, fname
