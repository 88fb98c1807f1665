"""cineSpace (.csp) files with a pre-LUT shaper on all three channels -- TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations


def write_csp_with_prelut(path, n, tab, shapers):
    """A 3D .csp of lattice `tab` [r, g, b, 3] (n^3, red fastest in the file) behind per-channel shapers (inputs, outputs),
    monotonic; points wrapped over several lines like real files."""
    with open(path, "w") as f:
        f.write("CSPLUTV100\n3D\n\nBEGIN METADATA\nshaper test\nEND METADATA\n\n")
        for xs, ys in shapers:
            f.write("%d\n" % len(xs))
            for vals in (xs, ys):
                for i in range(0, len(vals), 5):
                    f.write(" ".join("%.9g" % v for v in vals[i:i + 5]) + "\n")
        f.write("\n%d %d %d\n" % (n, n, n))
        f.write("".join("%.9g %.9g %.9g\n" % tuple(tab[r, g, b]) for b in range(n) for g in range(n) for r in range(n)))
