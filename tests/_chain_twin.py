"""Reference of the two-LUT pass -- TEST INFRASTRUCTURE ONLY.

The contract is a composition of existing pieces, no new arithmetic: stages 1 and 2 of the subsampling-change twin
(`tests._xsub_twin.lut_rgb`: YUV -> integer RGB at the input layout, then the C oracle's lut3d with the first LUT and its prelut),
the C oracle's lut3d again on those integer codes with the second LUT (`oracle.binding.apply_rgb`: its own size and scale, no
prelut), and stage 3 at the output layout (`oracle.lut3d_numpy.rgb_codes_to_yuv`).
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import rgb_codes_to_yuv
from tests import _xsub_twin as xsub

LAYOUTS = xsub.LAYOUTS
consts = xsub.consts


def lut_pairs(cube_dir, d):
    """The LUT pairs of the chain tests, files written into `d`: name -> (path of A, path of B, A's oracle prelut or None).
    A and B differ in size on purpose: it catches a kernel that reuses the first lattice's strides or scale.
      log709_random  a 33^3 technical LUT, then a 9^3 look with nodes outside [0, 1]
      wide_domain    a 9^3 A with nodes in [-0.25, 1.25] (its output is clipped), then a 17^3 B whose DOMAIN gives scale 0.5
      csp_random     a 17^3 .csp A behind a shaper (a prelut), then the 9^3 look"""
    from lut_renderer_amd import cube
    from tests._csp_files import write_csp_with_prelut
    cube.write_cube(d / "wide_9.cube", cube.identity_lattice(9) * 1.5 - 0.25)
    cube.write_cube(d / "domain_17.cube", cube.log709_lattice(17), domain_min=(0, 0, 0), domain_max=(2, 2, 2))
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    write_csp_with_prelut(d / "shaped.csp", 17, cube.log709_lattice(17), shapers)
    return {"log709_random": (cube_dir / "log709_33.cube", cube_dir / "random_9.cube", None),
            "wide_domain": (d / "wide_9.cube", d / "domain_17.cube", None),
            "csp_random": (d / "shaped.csp", cube_dir / "random_9.cube", orc.parse_lut_file_ex(d / "shaped.csp")[3])}


def second_lut(B, ib, dl, rgb):
    """lut3d of LUT `B` (anything with .table and .scale) on integer (R, G, B) codes at depth dl; returns (R, G, B)."""
    dt = np.uint8 if dl <= 8 else np.uint16
    r, g, b = [np.asarray(a).astype(dt) for a in rgb]
    go, bo, ro = orc.apply_rgb(B.table, B.scale, dl, ib, (g, b, r))
    return ro, go, bo


def intermediate(A, ia, k, dl, icsx, icsy, planes, prelut_a=None):
    """q1 of the contract: integer (R, G, B) at luma resolution after the first LUT, clipped to [0, 2^dl - 1]."""
    return xsub.lut_rgb(A.table, A.scale, ia, k, dl, icsx, icsy, planes, prelut_a)


def apply(A, B, ia, ib, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, prelut_a=None):
    """The contract: (Y, Cb, Cr) at the output depth and layout."""
    q1 = intermediate(A, ia, k, dl, icsx, icsy, planes, prelut_a)
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, second_lut(B, ib, dl, q1))
