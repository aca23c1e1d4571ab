#!/usr/bin/env python
"""Generate tests/golden/warp.npz by running the REAL reference ``resize_exr`` (``GenProjector/util.py:279-343``) on the CPU.

Run only where the reference checkout exists (see ``make_golden.py``); a second or two:

    python tests/golden/make_golden_warp.py

``GenProjector/util.py`` needs OpenEXR, cv2 and vtk to import, and the function hard-codes ``theta, phi, move = 0``.  So the
text span of the function is read at generation time, the line that assigns the three constants is found by a pattern and
replaced by each case's values, and the result is executed with numpy, math and a stand-in ``cv2`` whose ``remap`` returns
its two maps -- nothing of the text is stored.  The file holds OUTPUTS only: per case of ``tests/warp_oracle.py``
(``PARAMS`` x ``SHAPES``)

  <case>/row, <case>/col   the reference's float32 maps (``map_x`` = row, ``map_y`` = column), (h, w)
  <case>/d_ref             the worst chord distance between those maps and the float64 restatement
                           (``warp_oracle.positions``), both turned into unit vectors

The chord is used because the column alone is ill-conditioned at the poles: the reference's row 0 comes out shifted by
half a turn (``cos(float32(-pi/2)) < 0``), which is the same point of the sphere.
"""
import math
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EMLIGHT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CONSTANTS = re.compile(r"^(\s*)theta\s*,\s*phi\s*,\s*move\s*=[^\n]*$", re.M)


def function_text():
    text = open(os.path.join(REF, "GenProjector", "util.py")).read()
    span = re.search(r"^def resize_exr\(.*?(?=^def |\Z)", text, re.S | re.M)
    assert span, "resize_exr not found"
    assert len(CONSTANTS.findall(span.group(0))) == 1, "expected one assignment of theta, phi, move"
    return span.group(0)


def reference_maps(text, H, W, h, w, theta, phi, move):
    cv2 = types.SimpleNamespace(INTER_LINEAR=1, BORDER_WRAP=3,
                                remap=lambda img, map_col, map_row, interpolation, borderMode: (map_row, map_col))
    code = CONSTANTS.sub(lambda m: "%stheta, phi, move = %r, %r, %r" % (m.group(1), theta, phi, move), text)
    ns = {"np": np, "math": math, "cv2": cv2}
    exec(compile(code, "resize_exr", "exec"), ns)
    row, col = ns["resize_exr"](np.zeros((H, W, 3), dtype=np.float32), res_x=h, res_y=w)
    assert row.shape == col.shape == (h, w)
    return row.astype(np.float32), col.astype(np.float32)


def main():
    from tests import warp_oracle as oracle
    text = function_text()
    out, worst = {}, 0.0
    for k, (theta, phi, move) in enumerate(oracle.PARAMS):
        for shape in oracle.SHAPES:
            H, W, h, w = shape
            row, col = reference_maps(text, H, W, h, w, theta, phi, move)
            want_row, want_col = oracle.positions(H, W, h, w, theta, phi, move)
            d = oracle.chord(row, col, want_row, want_col, H, W)
            name = oracle.case_name(k, shape)
            out[name + "/row"], out[name + "/col"], out[name + "/d_ref"] = row, col, np.float64(d)
            worst = max(worst, d)
            print("%-22s theta %6.1f phi %6.1f move %4.1f: chord to the float64 restatement %.3e" % (name, theta, phi, move, d))
    assert worst <= 1e-4, "the restatement is not the reference's operator"
    path = os.path.join(HERE, "warp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, worst chord %.3e" % (path, os.path.getsize(path), worst))


if __name__ == "__main__":
    main()
