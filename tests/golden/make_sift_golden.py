#!/usr/bin/env python3
"""Regenerate the small SIFT fixtures in tests/golden/ (needs the reference
tree: oracle/build_ref.sh builds oracle/_ref/vlsift_tool from its VLFeat).

vlfeat_sift_<w>x<h>.{kp,u8}: the features (n x 4 float32: x, y, sigma, angle)
and RootSIFT descriptors (n x 128 uint8) that the reference's own extractor
gives on the blob-field image of seed 7, identity view, at each size below.
The 640 x 480 views are make_golden.py's vlfeat_view{0,1,2}.  161 x 97 is there
for the halving of odd widths and heights.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TOOL = os.path.join(ROOT, "oracle", "_ref", "vlsift_tool")
SIZES = [(160, 120), (96, 64), (161, 97)]
SEED = 7

if __name__ == "__main__":
    if not os.path.exists(TOOL):
        subprocess.run(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")], check=True)
    for w, h in SIZES:
        stem = os.path.join(HERE, f"vlfeat_sift_{w}x{h}")
        r = subprocess.run([TOOL, stem + ".u8", stem + ".kp", str(w), str(h), str(SEED), "0", "0", "0", "1"],
                           check=True, capture_output=True, text=True)
        print(f"{w}x{h}: {r.stdout.strip()} features")
