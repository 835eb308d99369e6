"""CPU: the SIFT structs of _abi.py against include/sfmcore.h (sizes and field
offsets, through a C program), and the defaults."""
import ctypes as C
import os
import subprocess

import _helpers as H

abi = H.abi

STRUCTS = {
    "sfm_sift_options": abi.SiftOptions,
    "sfm_sift_summary": abi.SiftSummary,
}


def test_struct_layouts_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sfmcore.h"', 'int main(void) {']
    expect = []
    for cname, cls in STRUCTS.items():
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {f}));')
            expect.append(getattr(cls, f).offset)
    lines += ['  return 0;', '}']
    src = tmp_path / "s.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(H.ROOT, "include"), "-I/opt/rocm/include", str(src), "-o",
                    str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect
    assert C.sizeof(abi.SiftOptions) == 32 and C.sizeof(abi.SiftSummary) == 48


def test_default_options():
    o = abi.SiftOptions()
    abi.load().sfm_sift_options_default(C.byref(o))
    assert (o.n_octaves, o.n_scales, o.first_octave, o.root_sift, o.orientation, o.reserved) == (6, 3, 0, 1, 1, 0)
    assert o.edge_threshold == 10.0 and abs(o.peak_threshold - 0.04) < 1e-8
    abi.load().sfm_sift_options_default(None)   # tolerated


def test_signatures_cover_the_new_symbols():
    names = {s[0] for s in abi.SIGNATURES}
    assert {"sfm_sift", "sfm_sift_host", "sfm_sift_options_default", "sfm_synth_image", "sfm_mvg_write_feat"} <= names
    assert not abi.load().missing_symbols
