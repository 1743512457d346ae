"""Shared inputs for the multi-consensus tests (CPU: test_multicons_twin, GPU:
test_multicons_gpu), each with the cluster sizes it gives: the reference
binary and the host pipeline agree on them byte for byte.

  tie sets      cons_cases.tie_set(L, depth): two noise-free haplotypes in
                equal numbers; -d2 gives two clusters of depth / 2. Depths 66
                and 130 need two-word and three-word read-id masks.
  hap sets      the generator of tests/test_multicons_cpu.py, restated: L =
                500, 6 SNPs per extra haplotype, an optional 3-base deletion,
                4 % noise, reads dealt round-robin over n_hap haplotypes.
  goldens       heter.fa, 3alleles.fa, seq.fa.
"""
import os
import random

import cons_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TIE_LENGTHS = (63, 64, 65, 129, 600)
TIE_DEPTHS = (4, 6, 8, 66, 130)

# (seed, n_hap, depth, max_n_cons) -> cluster sizes
HAP_CASES = {
    (1, 1, 24, 2): [12, 12],          # noise alone splits it
    (2, 1, 24, 2): [24],              # the single-cluster branch
    (7, 1, 24, 2): [24],
    (1, 2, 24, 2): [12, 12], (2, 2, 24, 2): [12, 12], (7, 2, 24, 2): [12, 12],
    (1, 2, 24, 3): [12, 12], (2, 2, 24, 3): [12, 12], (7, 2, 24, 3): [12, 12],
    (1, 3, 24, 3): [8, 8, 8], (7, 3, 24, 3): [8, 8, 8],
    (2, 3, 24, 3): [16, 8],           # k shrinks from 3 to 2
    (1, 1, 70, 2): [34, 36], (1, 2, 70, 2): [35, 35],
    (1, 3, 70, 3): [23, 23, 24], (1, 2, 70, 3): [35, 35],
    (2, 1, 70, 2): [70], (2, 2, 70, 2): [35, 35],
    (2, 3, 70, 3): [23, 24, 23], (2, 2, 70, 3): [35, 35],
    (7, 1, 70, 2): [70], (7, 2, 70, 2): [35, 35],
    (7, 3, 70, 3): [24, 23, 23], (7, 2, 70, 3): [35, 35],
}

# name -> (max_n_cons, cluster sizes)
GOLDEN_CASES = {
    "heter.fa": (2, [7, 8]),
    "3alleles.fa": (3, [40, 52, 34]),
    "seq.fa": (2, [7, 3]),
}


def hap_reads(seed, n_hap, L=500, depth=24, snps=6):
    """The reads of test_multicons_cpu._gen(seed, n_hap), as ACGT strings."""
    rng = random.Random(seed)
    base = "".join(rng.choice("ACGT") for _ in range(L))
    haps = [base]
    for _h in range(1, n_hap):
        hb = list(base)
        for p in rng.sample(range(10, L - 10), snps):
            hb[p] = rng.choice([c for c in "ACGT" if c != hb[p]])
        if rng.random() < 0.5:
            d = rng.randrange(20, L - 30)
            hb = hb[:d] + hb[d + 3:]
        haps.append("".join(hb))

    def noisy(h):
        out = []
        for ch in h:
            r = rng.random()
            if r < 0.02:
                out.append(rng.choice("ACGT"))
            elif r < 0.03:
                pass
            elif r < 0.04:
                out.extend((ch, rng.choice("ACGT")))
            else:
                out.append(ch)
        return "".join(out)

    return [noisy(haps[i % n_hap]) for i in range(depth)]


def encode(read):
    return bytes("ACGT".index(c) for c in read.upper())


def hap_set(seed, n_hap, depth=24):
    """One read set of codes 0..3, as msa_batch_results takes them."""
    return [encode(r) for r in hap_reads(seed, n_hap, depth=depth)]


def tie_cases():
    """[(name, reads as code bytes, cluster sizes at -d2)]"""
    return [("tie_l%d_d%d" % (length, depth), cons_cases.tie_set(length, depth), [depth // 2] * 2)
            for length in TIE_LENGTHS for depth in TIE_DEPTHS]


def read_fasta(path):
    """The reads of a FASTA file as ACGT strings."""
    reads, cur = [], None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            cur = []
            reads.append(cur)
        elif line:
            cur.append(line)
    return ["".join(parts).upper() for parts in reads]


def golden_set(name):
    return [encode(r) for r in read_fasta(os.path.join(GOLDEN, name))]


def write_fasta(path, reads):
    """reads: ACGT strings or code bytes."""
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            if not isinstance(r, str):
                r = "".join("ACGT"[c] for c in r)
            f.write(">r%d\n%s\n" % (i, r))
