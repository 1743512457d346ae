"""The seam differential harness on the CPU (abpoa_amd_seamtwin).

abamd_seam_test.c aligns every read with the oracle and with a device under
test on the same graph and compares the whole abpoa_res_t: best_score,
n_cigar, every CIGAR word, node_s/e, query_s/e, n_aln_bases, n_matched_bases.
tests/test_seam_gpu.py runs it with the GPU core as the device. Here the
device is the oracle again, behind a mutator that changes exactly one field of
one read's result, which proves two things without a GPU: the harness's own
loop (sort, band-state reset, windows, reverse strand, CIGAR reversal, fold)
is self-consistent, and its comparator fails on every field it claims to
compare.
"""
import os
import re
import subprocess

import pytest

from conftest import CSRC, GOLDEN, ORACLE_SO
import seam_cases as sc

SEAMTWIN = os.path.join(CSRC, "abpoa_amd_seamtwin")
OK_RE = re.compile(rb"^seam OK: (\d+) reads, (\d+) alignments, (\d+) cigar words compared$")


@pytest.fixture(scope="module")
def seamtwin(cputest_bin):
    if not os.path.exists(SEAMTWIN):
        subprocess.run(["make", "-j4", "cputest"], cwd=CSRC, check=True, stdout=subprocess.DEVNULL)
    return SEAMTWIN


@pytest.fixture(scope="module")
def synth13(tmp_path_factory):
    """--seed 91 --len 400 --depth 24 at 13 % error: the input of the GPU cases."""
    return sc.synth13(tmp_path_factory.mktemp("seam") / "s91.fa")


def _run(seamtwin, args):
    return subprocess.run([seamtwin, ORACLE_SO] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _counts(p):
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    m = OK_RE.match(p.stdout.splitlines()[-1])
    assert m, p.stdout
    return tuple(int(x) for x in m.groups())


def test_clean_on_seq_fa(seamtwin):
    # 10 reads: 9 whole-graph alignments
    reads, alns, words = _counts(_run(seamtwin, [os.path.join(GOLDEN, "seq.fa")]))
    assert (reads, alns) == (10, 9) and words > 9 * 40


def test_clean_on_synth13(seamtwin, synth13):
    reads, alns, words = _counts(_run(seamtwin, [synth13]))
    assert (reads, alns) == (24, 23) and words > 23 * 350


def test_clean_with_windows_strands_rev_cigar(seamtwin, synth13):
    # per read: the whole graph, 3 windows, the reverse strand
    reads, alns, words = _counts(_run(seamtwin, ["--windows", "3", "--both-strands", "--rev-cigar", synth13]))
    assert (reads, alns) == (24, 23 * 5) and words > 23 * 350


def test_clean_without_cigar(seamtwin, synth13):
    reads, alns, words = _counts(_run(seamtwin, ["--no-cigar", synth13]))
    assert (reads, alns, words) == (24, 23, 0)


# variant -> what the mismatch line must name
MUTATIONS = {
    "best_score": rb"field best_score:",
    "n_cigar": rb"field n_cigar:",
    "node_s": rb"field node_s:",
    "node_e": rb"field node_e:",
    "query_s": rb"field query_s:",
    "query_e": rb"field query_e:",
    "n_aln_bases": rb"field n_aln_bases:",
    "n_matched_bases": rb"field n_matched_bases:",
    "cigar_op": rb"field cigar\[\d+\] of \d+: op differs:",
    "cigar_node": rb"field cigar\[\d+\] of \d+: node differs:",
    "cigar_query": rb"field cigar\[\d+\] of \d+: query differs:",
}


@pytest.mark.parametrize("read", [1, 9])
@pytest.mark.parametrize("field", sorted(MUTATIONS))
def test_mutation_is_caught(seamtwin, field, read):
    """One changed field in one read's result: exit 1, that field and that
    read named, and nothing else reported."""
    p = _run(seamtwin, ["--mutate", "%s@%d" % (field, read), os.path.join(GOLDEN, "seq.fa")])
    assert p.returncode == 1, p.stdout
    lines = p.stdout.splitlines()
    bad = [l for l in lines if l.startswith(b"seam MISMATCH")]
    assert len(bad) == 1, p.stdout
    assert bad[0].startswith(b"seam MISMATCH read %d (whole graph, default) " % read), bad[0]
    assert re.search(MUTATIONS[field], bad[0]), bad[0]
    assert lines[-1].startswith(b"seam FAILED: 1 mismatches")


@pytest.mark.parametrize("read", [1, 9])
def test_mutation_of_last_word_alone_is_caught(seamtwin, read):
    p = _run(seamtwin, ["--mutate", "cigar_last@%d" % read, os.path.join(GOLDEN, "seq.fa")])
    assert p.returncode == 1, p.stdout
    bad = [l for l in p.stdout.splitlines() if l.startswith(b"seam MISMATCH")]
    assert len(bad) == 1, p.stdout
    m = re.search(rb"read %d \(whole graph, default\) field cigar\[(\d+)\] of (\d+):" % read, bad[0])
    assert m and int(m.group(1)) == int(m.group(2)) - 1, bad[0]


def test_mutation_in_reversed_cigar_is_caught(seamtwin):
    p = _run(seamtwin, ["--rev-cigar", "--mutate", "cigar_node@4", os.path.join(GOLDEN, "seq.fa")])
    assert p.returncode == 1 and b"read 4 (whole graph, default) field cigar[" in p.stdout, p.stdout


def test_harness_goes_on_after_a_mismatch(seamtwin, synth13):
    """A mismatch at read 2 does not end the run: all 23 alignments are made."""
    p = _run(seamtwin, ["--mutate", "best_score@2", synth13])
    assert p.returncode == 1
    assert p.stdout.splitlines()[-1].startswith(b"seam FAILED: 1 mismatches (24 reads, 23 alignments")


def test_unaligned_mutation_target_is_an_error(seamtwin):
    """A --mutate that never fired must not look like a pass."""
    p = _run(seamtwin, ["--mutate", "best_score@0", os.path.join(GOLDEN, "seq.fa")])
    assert p.returncode != 0 and b"never aligned" in p.stderr
