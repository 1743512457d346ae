"""Shared inputs for the consensus-twin tests (CPU: test_cons_twin, GPU:
test_cons_gpu): tie-stress read sets and row-count boundary sets.

A tie-stress set holds two noise-free haplotypes in equal numbers (reads
alternate A, B, A, B ...). The haplotypes differ by a SNP every ~25 bases and
by one 3-base deletion, so every variant site leaves two out-edges of EQUAL
weight with EQUAL downstream scores: the heaviest-bundle choice there is
decided purely by the tie rules (inner nodes: the later-scanned edge wins on
score >=; SRC: strictly higher weight, then strictly higher score).
Lengths 63/64/65/129 put the graphs' row counts on both sides of the 64-row
staging step of the reverse sweep.
"""
import numpy as np

TIE_LENGTHS = (63, 64, 65, 129)
TIE_DEPTHS = (2, 4)
# single-haplotype sets: rows = length + 2, i.e. exactly 64, 65, 128, 129, 130
CHAIN_LENGTHS = (62, 63, 126, 127, 128)


def haplotypes(length, seed):
    """(hapA, hapB) as uint8 code arrays (0..3)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, size=length, dtype=np.uint8)
    b = a.copy()
    # position 0 too: SRC itself then has two equal-weight out-edges
    for pos in [0] + list(range(12, length, 25)):
        b[pos] = (b[pos] + 1 + rng.integers(0, 3)) % 4   # always a different base
    cut = length // 2 + 3                                 # between two SNP sites
    b = np.concatenate([b[:cut], b[cut + 3:]])
    return a, b


def tie_set(length, depth, seed=None):
    """One read set: depth reads alternating hapA, hapB (bytes of codes)."""
    a, b = haplotypes(length, 1000 + length if seed is None else seed)
    return [(a if i % 2 == 0 else b).tobytes() for i in range(depth)]


def chain_set(length):
    """Two identical reads: a pure chain graph with length + 2 rows."""
    rng = np.random.default_rng(2000 + length)
    a = rng.integers(0, 4, size=length, dtype=np.uint8).tobytes()
    return [a, a]


def all_sets():
    """[(name, reads)] — every tie-stress and boundary set."""
    out = []
    for length in TIE_LENGTHS:
        for depth in TIE_DEPTHS:
            out.append(("tie_l%d_d%d" % (length, depth), tie_set(length, depth)))
    # a longer one: ~24 variant sites across several staging chunks
    out.append(("tie_l600_d4", tie_set(600, 4)))
    for length in CHAIN_LENGTHS:
        out.append(("chain_l%d" % length, chain_set(length)))
    return out


def write_fasta(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[c] for c in r)))
