"""The aligner seam on the GPU, field by field (-m gpu).

Every other GPU test of the DP kernels compares printed consensus and MSA
rows. abpoa_amd_seamgpu (abamd_seam_test.c) compares what the kernels return:
for every read it aligns with the oracle and with the GPU core on the same
graph and checks best_score, n_cigar, every packed CIGAR word, node_s/e,
query_s/e, n_aln_bases and n_matched_bases, then folds the oracle's result.
tests/test_seam_twin.py proves on the CPU that this comparator fails on each
of those fields.

Each case is one run on at most 1300 bases x 24 reads, states the score width
and, for the convex kernel, the instantiation it was written for, and asserts
both from what the harness prints (abamd_pick_width per alignment; fast or
generic as gpu_align.cpp decides it). The flags' effect on these inputs is
guarded in tests/test_seam_flags_cpu.py. Nothing here reads the reference
tree."""
import os
import re
import subprocess

import pytest

from conftest import CSRC, ORACLE_SO
import seam_cases as sc

pytestmark = pytest.mark.gpu

SEAMGPU = os.path.join(CSRC, "abpoa_amd_seamgpu")
N_READS = 24          # the 400 x 24 sets
N_ALN = N_READS - 1   # whole-graph alignments per pass


def seam(args):
    assert os.path.exists(SEAMGPU), "abpoa_amd_seamgpu not built (run __graft_entry__.build())"
    try:
        p = subprocess.run([SEAMGPU, ORACLE_SO] + [str(a) for a in args],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.exit("abpoa_amd_seamgpu hung on %r: nothing more is started on this GPU" % (args,), 3)
    out = p.stdout.decode()
    if p.returncode < 0 or p.returncode in (134, 139) or b"HIP error" in p.stderr:
        # a GPU fault or an abort, not a mismatch: end the session here
        pytest.exit("abpoa_amd_seamgpu died (%d) on %r: %s" % (p.returncode, args, p.stderr.decode()[-600:]), 3)
    assert p.returncode == 0, out + p.stderr.decode()[-2000:]
    r = {}
    m = re.search(r"^seam OK: (\d+) reads, (\d+) alignments, (\d+) cigar words compared$", out, re.M)
    assert m, out
    r["reads"], r["alns"], r["words"] = (int(x) for x in m.groups())
    m = re.search(r"^seam widths: int16 (\d+), int32 (\d+)$", out, re.M)
    r["i16"], r["i32"] = (int(x) for x in m.groups())
    m = re.search(r"^seam convex instantiation: fast (\d+), generic (\d+)$", out, re.M)
    r["fast"], r["generic"] = (int(x) for x in m.groups())
    r["longest_ins"] = int(re.search(r"^seam longest insertion: (\d+)$", out, re.M).group(1))
    r["batch_picks"] = [int(x) for x in re.findall(r"^seam batch job \d+: .* picks int(\d+)$", out, re.M)]
    m = re.search(r"^seam batch launch: (\d+) jobs at int(\d+)$", out, re.M)
    r["launch"] = (int(m.group(1)), int(m.group(2))) if m else None
    print(out.strip().splitlines()[-4:])
    return r


def check(r, reads, alns, width, fast=0, generic=0):
    """reads and alignments as the case expects, CIGAR words compared, every
    alignment at `width`, and the convex alignments split fast/generic as stated."""
    assert (r["reads"], r["alns"]) == (reads, alns), r
    assert r["words"] > 0, r
    assert (r["i16"], r["i32"]) == ((alns, 0) if width == 16 else (0, alns)), r
    assert (r["fast"], r["generic"]) == (fast, generic), r


@pytest.fixture(scope="module")
def s91(tmp_path_factory):
    return sc.synth13(tmp_path_factory.mktemp("seam") / "s91.fa")


# -z 100 ends alignments early only against the x45 scores (int32); at int16 it
# never fires on this input and -z 5 is the z-drop that does, in all three gap
# modes (tests/test_seam_flags_cpu.py guards both)
MODES = {"global": [], "local": ["-m", "1"], "extend": ["-m", "2"],
         "extend-z100": ["-m", "2", "-z", "100"], "extend-z5": ["-m", "2", "-z", "5"]}


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_gap_and_alignment_modes(s91, gap, mode, width):
    """Three gap modes x global/local/extension (and two z-drops) x both widths,
    each read aligned under the default, ABPOA_AMD_DP_GENERIC=1 and
    ABPOA_AMD_DP_RING=1. Convex global runs the fast instantiation in the
    default setting only; every other convex alignment is generic."""
    scoring = sc.GAPS[gap] if width == 16 else sc.GAPS_X45[gap]
    r = seam(scoring + MODES[mode] + ["--settings", s91])
    if gap != "convex":
        check(r, N_READS, 3 * N_ALN, width)
    elif mode == "global":
        check(r, N_READS, 3 * N_ALN, width, fast=N_ALN, generic=2 * N_ALN)
    else:
        check(r, N_READS, 3 * N_ALN, width, generic=3 * N_ALN)


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_path_scores(gap, width):
    """-G (inc_path_score): pre_ps in the gather and in all three backtracks.
    It must select the generic convex kernel in every setting."""
    scoring = sc.GAPS[gap] if width == 16 else sc.GAPS_X45[gap]
    r = seam(scoring + ["-G", "--settings", sc.SYNTH13_SEED1])
    check(r, N_READS, 3 * N_ALN, width, generic=3 * N_ALN if gap == "convex" else 0)


PLACEMENT = {"R": ["-R"], "J": ["-J"], "RJ": ["-R", "-J"], "e5-extend": ["-e", "5", "-m", "2"]}


@pytest.mark.parametrize("flags", list(PLACEMENT))
@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_gap_placement_and_bonus(s91, gap, flags):
    """-R / -J reorder the backtrack's branches; -e 5 -m2 is extension mode
    with an end bonus (which the reference parses and never reads). int16;
    global convex is the fast instantiation, extension the generic one."""
    r = seam(sc.GAPS[gap] + PLACEMENT[flags] + [s91])
    if gap != "convex":
        check(r, N_READS, N_ALN, 16)
    elif flags == "e5-extend":
        check(r, N_READS, N_ALN, 16, generic=N_ALN)
    else:
        check(r, N_READS, N_ALN, 16, fast=N_ALN)


@pytest.mark.parametrize("gap", ["convex", "affine"])
def test_subgraph_windows(s91, gap):
    """--windows 4: per read the whole graph and 4 subgraphs away from SRC and
    SINK (reachability map, compact rows, row_node_id mapping of pack_job)."""
    r = seam(sc.GAPS[gap] + ["--windows", "4", s91])
    check(r, N_READS, 5 * N_ALN, 16, fast=5 * N_ALN if gap == "convex" else 0)


@pytest.mark.parametrize("gap", ["convex", "affine"])
def test_both_strands(s91, tmp_path, gap):
    """Every third read is reverse-complemented in the file and every read is
    aligned on both strands, as -s does: best_score of a poor alignment."""
    fa = sc.every_third_reversed(s91, tmp_path / "rc.fa")
    r = seam(sc.GAPS[gap] + ["--both-strands", fa])
    check(r, N_READS, 2 * N_ALN, 16, fast=2 * N_ALN if gap == "convex" else 0)


@pytest.mark.parametrize("gap", ["convex", "linear"])
def test_rev_cigar(s91, gap):
    r = seam(sc.GAPS[gap] + ["--rev-cigar", s91])
    check(r, N_READS, N_ALN, 16, fast=N_ALN if gap == "convex" else 0)


@pytest.mark.parametrize("gap", ["convex", "linear"])
def test_no_cigar(s91, gap):
    """ret_cigar = 0: best_score alone, and n_cigar == 0."""
    r = seam(sc.GAPS[gap] + ["--no-cigar", s91])
    assert (r["reads"], r["alns"], r["words"]) == (N_READS, N_ALN, 0), r
    assert (r["i16"], r["i32"]) == (N_ALN, 0), r
    assert (r["fast"], r["generic"]) == ((N_ALN, 0) if gap == "convex" else (0, 0)), r


@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_tiny_graphs(tmp_path, gap):
    """Reads of 1, 2 and 3 bases: the rolled-load clamps sit here."""
    files = [sc.write_fasta(tmp_path / ("t%d.fa" % i), pair)
             for i, pair in enumerate([("A", "A"), ("AC", "AG"), ("ACG", "ATG")])]
    r = seam(sc.GAPS[gap] + ["--settings"] + files)
    check(r, 6, 9, 16, fast=3 if gap == "convex" else 0, generic=6 if gap == "convex" else 0)


@pytest.mark.parametrize("band", ["-1", "1200"])
def test_insertion_past_the_f_window(tmp_path, band):
    """600- and 1100-base insertions against a 120-base graph: the convex
    backtrack recomputes F in 512-cell windows, so the 600-base walk needs a
    second window; the later reads align along branches longer than the row
    ring. Unbanded rows are generic; -b 1200 is banded, so fast by default."""
    fa = sc.long_insertion(tmp_path / "ins.fa")
    r = seam(["-b", band, "--settings", fa])
    if band == "-1":
        check(r, 6, 15, 16, generic=15)
    else:
        check(r, 6, 15, 16, fast=5, generic=10)
    assert r["longest_ins"] >= 600, r   # more than one 512-cell window
    r = seam(sc.GAPS["affine"] + ["-b", band, fa])   # affine stores F
    check(r, 6, 5, 16)
    assert r["longest_ins"] >= 600, r   # more than one 512-cell window


def test_mixed_width_batch(tmp_path):
    """One abamd_gpu_align_batch launch whose jobs pick int16 and int32: the
    launch runs at the widest type. With -M 30 -E 30,15 the rule says int16 up
    to max(qlen, rows) * 30 + 60 <= 32242, i.e. 1072 rows. The picks are the
    rule's own answers (abamd_pick_width), printed by the harness: every read
    of the 300 and 700 sets aligns at int16 and every read of the 1300 set at
    int32, while the batch jobs run against the FINAL graphs, and that of the
    700 set has grown past 1072 rows: int16, int32, int32."""
    files = []
    for length in (300, 700, 1300):
        files.append(sc.synth(tmp_path / ("b%d.fa" % length), length, length, 8, rates=None))
    r = seam(["-M", "30", "-X", "60", "-O", "60,360", "-E", "30,15", "--batch"] + files)
    assert (r["reads"], r["alns"]) == (24, 3 * 7 + 3) and r["words"] > 0, r
    assert r["batch_picks"] == [16, 32, 32] and r["launch"] == (3, 32), r
    assert (r["i16"], r["i32"]) == (14, 7), r
    assert (r["fast"], r["generic"]) == (3 * 7, 0), r


@pytest.mark.parametrize("gap", ["convex", "affine"])
def test_amino_acid_alphabet(tmp_path, gap):
    """m = 27 with BLOSUM62, 300 residues x 10 reads."""
    fa = sc.amino(tmp_path / "aa.fa")
    r = seam(["-c", "-t", sc.BLOSUM] + sc.GAPS[gap] + ["--settings", fa])
    check(r, 10, 27, 16, fast=9 if gap == "convex" else 0, generic=18 if gap == "convex" else 0)
