"""The arena-overflow inputs do overflow (no GPU needed).

The product drivers reserve rows * (2w + 160) + qlen + 64 DP cells per job and
retry a job whose adaptive band outgrows that with twice the reservation. No
knob shrinks the reservation, so tests/test_resident_paths_gpu.py forces the
retry with real inputs (batch_cases.overflow_set). This measures them with the
oracle, which counts the banded cells per plane of each alignment
(abpoa_amd_seamtwin --cells): D1 must need more than the reservation and fit
twice it; D2 must need more than twice it and fit four times it, so that its
retry overflows again exactly once. The GPU test's expected counter values
follow from these figures. Measured (convex / affine / linear), reads 2-4:
  D1  oracle 528632-533127 / 535627-539316 / 502616-541302 cells,
      est 337665-344395, ratio 1.47-1.61
  D2  oracle 987929-1016805 / 1018604-1023463 / 981997-1023674 cells,
      est 405607-409334, ratio 2.41-2.52"""
import os
import re
import subprocess

import pytest

from conftest import CSRC, ORACLE_SO
import batch_cases as bc

TWIN = os.path.join(CSRC, "abpoa_amd_seamtwin")
LINE = re.compile(r"^seam cells read (\d+): rows (\d+) qlen (\d+) oracle (\d+) est (\d+) n_cigar (\d+)$", re.M)


def cells(fa, opts):
    p = subprocess.run([TWIN, ORACLE_SO, "--cells"] + opts + [fa], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout.decode()[-1000:] + p.stderr.decode()[-1000:]
    return [tuple(int(x) for x in m.groups()) for m in LINE.finditer(p.stdout.decode())]


@pytest.mark.parametrize("gap", ["convex", "affine", "linear"])
def test_overflow_inputs_overflow(cputest_bin, tmp_path, gap):
    d1 = cells(bc.overflow_set(tmp_path, "D1"), bc.GAPS[gap])
    d2 = cells(bc.overflow_set(tmp_path, "D2"), bc.GAPS[gap])
    assert len(d1) == 4 and len(d2) == 4
    for name, rows in (("D1", d1), ("D2", d2)):
        for read, n_rows, qlen, oracle, est, _n in rows:
            print("%s %s read %d: rows %d qlen %d oracle %d est %d ratio %.2f"
                  % (name, gap, read, n_rows, qlen, oracle, est, oracle / est))
    # what the issue asks for
    assert any(oracle > est for _r, _n, _q, oracle, est, _c in d1)
    assert any(oracle > 2 * est for _r, _n, _q, oracle, est, _c in d2)
    # what the GPU test's exact counters rest on: read 1 carries the insertion
    # and fits; reads 2-4 lack it and overflow once (D1) or twice (D2)
    assert d1[0][3] <= d1[0][4] and d2[0][3] <= d2[0][4]
    assert all(est < oracle <= 2 * est for _r, _n, _q, oracle, est, _c in d1[1:])
    assert all(2 * est < oracle <= 4 * est for _r, _n, _q, oracle, est, _c in d2[1:])


def test_no_input_gives_an_empty_cigar(cputest_bin, tmp_path):
    """The candidate for ABAMD_FOLD_NOOP: a poly-A read
    against a C/G/T graph aligns nowhere in any mode, and the backtrack still
    reports one word, the whole read as an insertion (two in extension mode)."""
    fa = bc.unaligned_set(tmp_path)
    for opts in (["-m1"], ["-m2"], [], ["-m1"] + bc.AFFINE, ["-m1"] + bc.LINEAR):
        n = [c[5] for c in cells(fa, opts)]
        assert len(n) == 5 and n[2] in (1, 2) and min(n) >= 1, (opts, n)
