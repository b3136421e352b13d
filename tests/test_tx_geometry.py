"""The transposition-exchange geometry (csrc/lpp_txgeom.h) without a GPU: tests/host/tx_geometry_main.cpp, built as a stand-alone host
program with the address and undefined-behaviour sanitizers, against the arithmetic of include/lpp_engine.h worked by hand:
per = ceil(N_down / P), peru = xchg_chunk / per; valid: xchg_chunk == per * peru and peru * P >= N_up; mult16: peru % 16 == 0;
fits32: P * per * peru <= 2^31 - 1."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n_up, n_dn, P, chunk) -> per, peru, requested, valid, mult16, fits32
CASES = [
    ((70, 70, 2, 1680), (35, 48, 1, 1, 1, 1)),  # lpp_xchg_chunk(70, 70, 2): 35 * 48, 96 >= 70
    ((70, 70, 2, 560), (35, 16, 1, 0, 1, 1)),  # 16 up indices per rank: 32 < 70
    ((924, 495, 4, 124 * 240), (124, 240, 1, 1, 1, 1)),  # ceil(495 / 4) = 124, 960 >= 924
    ((70, 70, 2, 0), (35, 0, 0, 0, 0, 0)),  # no chunk: the all-gather exchange, nothing else is worked out
    ((70, 70, 1, 1680), (70, 24, 1, 0, 0, 1)),  # one rank: 24 < 70, 24 % 16 = 8
    ((1, 1, 2, 16), (1, 16, 1, 1, 1, 1)),  # a padded rank: per = 1 covers the one down configuration
]


def test_tx_geometry_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tx_geometry")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "lanczosplusplus_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "tx_geometry_main.cpp")], check=True)
    args = [str(v) for case, _ in CASES for v in case]
    out = subprocess.run([exe] + args, check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(out) == len(CASES)
    for line, (case, want) in zip(out, CASES):
        head, rest = line.split(": ", 1)
        assert tuple(int(v) for v in head.split()) == case
        fields = dict(f.split("=", 1) for f in rest.split(" reason=")[0].split())
        got = tuple(int(fields[k]) for k in ("per", "peru", "requested", "valid", "mult16", "fits32"))
        assert got == want, line
        assert (rest.split(" reason=")[1] == "") == bool(want[3]), line  # a reason exactly when the geometry is not valid
