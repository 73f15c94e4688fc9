"""The one rule for the identity padding below the last real row (csrc/chol_schedule.h, real_rows) through a sanitised host program.
The one-launch Cholesky's row tiles and the triangular inverse skip the 16-row sub-tiles this rule calls padding."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_real_rows_table(tmp_path):
    """real_rows(n_real, row0, rows): the rows of the tile [row0, row0 + rows) below n_real = n + R, rounded up to whole 16-row sub-tiles and
    clipped to the tile.  The table is written by hand: n_real rows into one 64-row tile (0, 1, 15, 16, 17, 63, 64 and more), R = 1 and
    R = 3 on the same design, the last row tiles of n = 2000, 5000 and 16000 (NP = 2048, 5120, 16128), and a 128-row tile."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "real_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", "real_rows_check.cpp"),
                           "-o", exe])
    # (n_real, row0, rows) -> real rows
    cases = [
        # n_real - row0 rows of a 64-row tile are real
        ((128, 128, 64), 0),            # 0: the tile starts at the first padding row
        ((129, 128, 64), 16),           # 1
        ((143, 128, 64), 16),           # 15
        ((144, 128, 64), 16),           # 16: exactly one sub-tile
        ((145, 128, 64), 32),           # 17
        ((191, 128, 64), 64),           # 63
        ((192, 128, 64), 64),           # 64
        ((1000, 128, 64), 64),          # the matrix goes on below the tile
        ((100, 128, 64), 0),            # the tile lies wholly behind the real rows
        ((0, 0, 64), 0),                # an empty matrix
        ((160, 128, 64), 32),           # 32
        ((161, 128, 64), 48),           # 33
        ((176, 128, 64), 48),           # 48
        ((177, 128, 64), 64),           # 49
        # R = 1 against R = 3 on n = 270 (NP = 384): tile 4 covers rows 256 .. 319
        ((271, 256, 64), 16),           # 15 rows
        ((273, 256, 64), 32),           # 17 rows: the second sub-tile holds right-hand sides only
        ((271, 320, 64), 0),
        ((273, 320, 64), 0),
        # R = 1 against R = 3 where the targets start a new block: n = 256
        ((257, 256, 64), 16),
        ((259, 256, 64), 16),
        # n = 2000, NP = 2048: tile 31 = rows 1984 .. 2047 holds 16 data rows and the target row
        ((2001, 1984, 64), 32),
        ((2001, 1920, 64), 64),
        ((2003, 1984, 64), 32),         # R = 3: 19 rows
        # n = 5000, NP = 5120: tile 78 = rows 4992 .. 5055 holds 9 real rows, tile 79 none
        ((5001, 4992, 64), 16),
        ((5001, 5056, 64), 0),
        # n = 16000, NP = 16128: tiles 250, 251 = the last block column, one real row
        ((16001, 16000, 64), 16),
        ((16001, 16064, 64), 0),
        ((16001, 15936, 64), 64),
        # the 128-row tiles of the triangular inverse's upper levels
        ((2001, 1920, 128), 96),
        ((5001, 4992, 128), 16),
        ((16001, 16000, 128), 16),
        ((2049, 2048, 128), 16),
        ((2049, 1920, 128), 128),
    ]
    text = "".join("%d %d %d\n" % c for c, _ in cases)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [int(x) for x in out.stdout.split()]
    assert len(got) == len(cases)
    for (case, want), g in zip(cases, got):
        assert g == want, (case, want, g)
