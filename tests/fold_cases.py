"""Inputs shared by tests/test_fold_round_gpu.py (the production fold kernel's
outputs against the flat twin, per round), tests/test_fold_round_twin.py (the
comparison's CPU self-test) and tests/test_fold_twin.py (the twin against the
pointer graph on the same inputs).

The inputs are small: the point is the graph's shape, not load. Every maker is
deterministic and returns the path(s) of the FASTA it wrote."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cons_cases as cc  # noqa: E402
import seam_cases as sc  # noqa: E402

# repeated offsets: their first edges grow heavier than their neighbours', so
# a weight sort over the wide node has to reorder, not only to append
STAIR_REPEATS = [35, 35, 35, 50, 50]


def _ref(seed, length):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(length))


def prefix_staircase(dirpath):
    """Reads ref[k:], k = 0..70, of a 200-base reference, then k = 35 three
    times and k = 50 twice: read k starts one base later than read k - 1, so
    SRC gains one out-edge per read and its degree passes through 64 and 65,
    the edge of the fold kernel's private-array sort, one read at a time.
    76 reads: two read-id words."""
    ref = _ref(4101, 200)
    reads = [ref[k:] for k in range(71)] + [ref[k:] for k in STAIR_REPEATS]
    return sc.write_fasta(os.path.join(str(dirpath), "stair_prefix.fa"), reads)


def suffix_staircase(dirpath):
    """Reads ref[:L - k], k = 0..110, of a 260-base reference, plus the same
    repeats: every read ends one base earlier, so SINK gains in-edges. (Not
    one per read: a short read's last bases can align a few columns off. The
    200-base variant with k <= 70 reaches 55 in-edges only; this one 86.)"""
    ref = _ref(4102, 260)
    L = len(ref)
    reads = [ref[:L - k] for k in range(111)] + [ref[:L - k] for k in STAIR_REPEATS]
    return sc.write_fasta(os.path.join(str(dirpath), "stair_suffix.fa"), reads)


# two identical reads of n bases: a chain graph of n + 2 rows — both sides of
# the 64-row steps of the CSR prefix scan and of the remain chunks
CHAIN_ROWS = (3, 63, 64, 65, 127, 128, 129)


def chain_sets(dirpath):
    paths = []
    for rows in CHAIN_ROWS:
        n = rows - 2
        read = _ref(4200 + n, n)
        paths.append(sc.write_fasta(os.path.join(str(dirpath), "chain_r%d.fa" % rows), [read, read]))
    return paths


def tie_sets(dirpath):
    """cons_cases.all_sets(): equal-weight edge pairs at every variant site."""
    paths = []
    for name, reads in cc.all_sets():
        p = os.path.join(str(dirpath), name + ".fa")
        cc.write_fasta(p, reads)
        paths.append(p)
    return paths


def bubble(dirpath):
    """A 300-base reference, and a 150-base insertion at position 150 carried
    by every other of 8 reads: the edge that skips the bubble has its
    successor more than two 64-row chunks away, next to in-chunk ones."""
    ref = _ref(4301, 300)
    ins = _ref(4302, 150)
    carrier = ref[:150] + ins + ref[150:]
    reads = [carrier if i % 2 == 0 else ref for i in range(8)]
    return sc.write_fasta(os.path.join(str(dirpath), "bubble.fa"), reads)


def amino(dirpath):
    """seam_cases.amino: 10 reads x 300 residues; with BLOSUM62 m = 27."""
    return sc.amino(os.path.join(str(dirpath), "aa.fa"))


AA_OPTS = ["-c", "-t", sc.BLOSUM, "-O", "4", "-E", "2"]


def low_alpha(dirpath):
    """20 reads x 500 bases at make_synth's 10 % error: with
    ABPOA_AMD_NODE_ALPHA=0.02 the planned pools are too small and grow."""
    return sc.synth(os.path.join(str(dirpath), "d20_l500.fa"), 77, 500, 20, rates=None)


def parse_fold_check(stderr):
    """The harness's [fold-check] line: ints by key, rows_by_set as a list."""
    lines = [ln for ln in stderr.decode().splitlines() if ln.startswith("[fold-check] ")]
    assert len(lines) == 1, stderr.decode()[-2000:]
    d = {}
    for kv in lines[0].split()[1:]:
        k, v = kv.split("=")
        d[k] = [int(x) for x in v.split(",")] if k == "rows_by_set" else int(v)
    return d


def n_reads(path):
    return sum(1 for ln in open(path) if ln.startswith(">"))
