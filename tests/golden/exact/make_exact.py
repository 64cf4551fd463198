#!/usr/bin/env python3
"""Writes tests/golden/exact/*.npz: the inputs a formula does not reproduce and the exact (200-bit mpmath,
tests/exact_ref.py) closures, tendencies, boundary fluxes and bounds of every fixture, rounded to Float64.

  python tests/golden/exact/make_exact.py [name ...]        (CPU only; needs mpmath)

tests/test_exact_reference.py regenerates every file and compares bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_ref as X  # noqa: E402

LIMIT = 64 * 1024


def main():
    names = sys.argv[1:] or X.fixture_names()
    for name in names:
        fx = X.build_fixture(name, generate=True)
        arrays = X.fixture_arrays(fx)
        np.savez_compressed(fx.path, **arrays)
        size = os.path.getsize(fx.path)
        assert size <= LIMIT, (name, size)
        print(f"{name}: {size} bytes")


if __name__ == "__main__":
    main()
