"""The device multi-consensus stage on the CPU (abpoa_amd_multiconstwin).

abamd_multicons_twin_test.c runs, after every read and with one lane over the
flat graph, what the resident batch driver runs on the GPU under
ABPOA_AMD_DEVICE_MULTICONS: rank/place, the het scan, abamd_read_clu_from_msa
on the compact matrix, abamd_flat_cons_phased_clu per cluster,
abamd_cons_from_paths, and with -r2 the consensus rows. It compares every
field with abpoa_generate_consensus / abpoa_generate_rc_msa on the live
pointer graph, the candidate list with a brute-force count, and the clusters
from the compact matrix with those from the full one. --mutate proves that
the comparison fails on the fields it claims to compare.
"""
import os
import re
import subprocess

import pytest

from conftest import CSRC, GOLDEN, ORACLE_SO
import multicons_cases as mc

TWIN = os.path.join(CSRC, "abpoa_amd_multiconstwin")
OK_RE = re.compile(rb"^multicons twin OK \((\d+) reads, (\d+) nodes, -d(\d), max (\d) clusters, "
                   rb"(\d+) clusters, (\d+) candidate columns, (\d+) consensus bases, "
                   rb"(\d+) row bytes compared\)$")


@pytest.fixture(scope="module")
def twin(cputest_bin):
    if not os.path.exists(TWIN):
        subprocess.run(["make", "-j4", "cputest"], cwd=CSRC, check=True, stdout=subprocess.DEVNULL)
    return TWIN


def _run(twin, args):
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    return subprocess.run([twin] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _ok(p):
    """(final cluster sizes, counters of the OK line)"""
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    lines = p.stdout.splitlines()
    m = OK_RE.match(lines[-1])
    assert m, p.stdout
    assert lines[-2].startswith(b"clusters ")
    return [int(x) for x in lines[-2].split()[1:]], [int(x) for x in m.groups()]


@pytest.mark.parametrize("rows", [[], ["-r2"]], ids=["cons", "r2"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("name", sorted(mc.GOLDEN_CASES))
def test_goldens(twin, name, d, rows):
    sizes, c = _ok(_run(twin, [os.path.join(GOLDEN, name), "-d", str(d)] + rows))
    want_d, want = mc.GOLDEN_CASES[name]
    if d == want_d:
        assert sizes == want
    assert c[5] > 0 and c[6] > 0
    assert (c[7] > 0) == bool(rows)


@pytest.mark.parametrize("name,reads,want", mc.tie_cases(), ids=[t[0] for t in mc.tie_cases()])
def test_tie_sets(twin, tmp_path, name, reads, want):
    """Equal-weight, equal-score choices at every variant site, under masks of
    one, two and three words; rows on the small depths."""
    fa = str(tmp_path / "tie.fa")
    mc.write_fasta(fa, reads)
    sizes, c = _ok(_run(twin, [fa, "-d", "2"] + (["-r2"] if len(reads) <= 8 else [])))
    assert sizes == want
    assert c[3] == 2


@pytest.mark.parametrize("case", sorted(mc.HAP_CASES), ids=lambda c: "seed%d_hap%d_depth%d_d%d" % c)
def test_hap_sets(twin, tmp_path, case):
    seed, n_hap, depth, d = case
    fa = str(tmp_path / "hap.fa")
    mc.write_fasta(fa, mc.hap_reads(seed, n_hap, depth=depth))
    sizes, c = _ok(_run(twin, [fa, "-d", str(d)] + (["-r2"] if depth == 24 else [])))
    assert sizes == mc.HAP_CASES[case]


PATHS_RE = re.compile(rb"^clustering paths: wide-partition (\d+) short-seed (\d+)$")


@pytest.mark.parametrize("case", [(1, 2, 24, 3), (2, 3, 24, 3), (1, 2, 70, 3)],
                         ids=lambda c: "seed%d_hap%d_depth%d_d%d" % c)
def test_clustering_paths_the_reference_leaves_undefined(twin, tmp_path, case):
    """Partial graphs of the -d3 sets reach both places where the clustering
    departs from the reference because the reference is undefined there:
    collect_1medoid over more than 20 het columns (its partition numbering
    overflows an int) and fewer medoids seeded than clusters asked for (it
    reads the unset ones). The twin must run clean through them — a wild
    index or an overflow would crash it or split compact from full — and say
    that it met them."""
    seed, n_hap, depth, d = case
    fa = str(tmp_path / "hap.fa")
    mc.write_fasta(fa, mc.hap_reads(seed, n_hap, depth=depth))
    p = _run(twin, [fa, "-d", str(d)])
    sizes, _c = _ok(p)
    assert sizes == mc.HAP_CASES[case]
    m = PATHS_RE.match(p.stdout.splitlines()[-3])
    assert m, p.stdout
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0, p.stdout


def test_d2_never_takes_those_paths(twin):
    """With two clusters asked for, seeding yields two medoids or none and
    collect_1medoid is never called: the default -d2 results cannot have
    changed."""
    p = _run(twin, [os.path.join(GOLDEN, "heter.fa"), "-d", "2"])
    _ok(p)
    assert PATHS_RE.match(p.stdout.splitlines()[-3]).groups() == (b"0", b"0")


MUTATIONS = ["n_cons", "clu_read_ids", "cons_base", "cons_cov", "cons_row"]


@pytest.mark.parametrize("field", MUTATIONS)
def test_mutation_is_caught(twin, field):
    """One changed field of the built result after the last read: exit 1 and
    that field named, after every earlier read compared clean."""
    p = _run(twin, [os.path.join(GOLDEN, "heter.fa"), "-d", "2", "-r2", "--mutate", field])
    assert p.returncode == 1, p.stdout + p.stderr
    bad = [l for l in p.stdout.splitlines() if l.startswith(b"MULTICONS TWIN MISMATCH")]
    assert len(bad) == 1, p.stdout
    assert bad[0].startswith(b"MULTICONS TWIN MISMATCH after read 14 "), bad[0]
    assert bad[0].endswith(b"field " + field.encode()), bad[0]


def test_mutation_that_cannot_apply_is_an_error(twin):
    p = _run(twin, [os.path.join(GOLDEN, "heter.fa"), "-d", "2", "--mutate", "cons_row"])
    assert p.returncode == 2 and b"needs -r2" in p.stderr


def test_cpu_library_reports_zero_multicons_stats(twin):
    import ctypes
    lib = ctypes.CDLL(os.path.join(CSRC, "libabpoa_amd_cputest.so"))
    v = [ctypes.c_uint64(7) for _ in range(8)]
    lib.abpoa_amd_get_multicons_stats.restype = None
    lib.abpoa_amd_get_multicons_stats(*[ctypes.byref(x) for x in v])
    assert [x.value for x in v] == [0] * 8
    lib.abpoa_amd_reset_multicons_stats.restype = None
    lib.abpoa_amd_reset_multicons_stats()
