"""Inputs and flag sets shared by tests/test_seam_gpu.py (the GPU core against
the oracle, field by field) and tests/test_seam_flags_cpu.py (the guards that
each flag changes the oracle's output on the input it is tested on)."""
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOSUM = os.path.join(GOLDEN, "BLOSUM62.mtx")
# --seed 1 --len 400 --depth 24 at 13 % error, committed: the first seed on
# which affine -G changes the reference's output
SYNTH13_SEED1 = os.path.join(GOLDEN, "synth13_seed1.fa")

GAPS = {"convex": [], "affine": ["-O", "4", "-E", "2"], "linear": ["-O", "0", "-E", "2"]}
# default scoring times 45: 400 bases x 90 > INT16_MAX, so the width pick says int32
GAPS_X45 = {"convex": ["-M", "90", "-X", "180", "-O", "180,1080", "-E", "90,45"],
            "affine": ["-M", "90", "-X", "180", "-O", "180", "-E", "90"],
            "linear": ["-M", "90", "-X", "180", "-O", "0", "-E", "90"]}
GAP_IDS = ["convex", "affine", "linear"]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def synth(path, seed, length, depth, rates=("0.06", "0.04", "0.03")):
    """make_synth.py; rates = (sub, del, ins), None for its 10 % defaults."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "make_synth.py"), str(path),
           "--seed", str(seed), "--len", str(length), "--depth", str(depth)]
    if rates:
        cmd += ["--sub", rates[0], "--del", rates[1], "--ins", rates[2]]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return str(path)


def synth13(path, seed=91, length=400, depth=24):
    """13 % error: rows with more predecessors than the kernels prefetch."""
    return synth(path, seed, length, depth)


def restore_inputs(tmp_path, dump_cmd):
    """For -i: the 13 % set split into its first 6 reads and the other 18;
    dump_cmd(first_fa) returns the -r4 dump of the first part. Returns
    (dump path, path of the other 18 reads)."""
    reads = read_fasta(synth13(tmp_path / "all.fa"))
    first = write_fasta(tmp_path / "first.fa", reads[:6])
    rest = tmp_path / "rest.fa"
    with open(rest, "w") as f:
        for i, r in enumerate(reads[6:]):
            f.write(">s%d\n%s\n" % (i, r))
    dump = tmp_path / "restore.gfa"
    dump.write_bytes(dump_cmd(first))
    return str(dump), str(rest)


def read_fasta(path):
    return [l.strip() for l in open(path) if not l.startswith(">")]


def write_fasta(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    return str(path)


def every_third_reversed(src, dst):
    """Reads 2, 5, 8, ... reverse-complemented (never the seeding read)."""
    reads = read_fasta(src)
    for i in range(2, len(reads), 3):
        reads[i] = "".join(COMP[c] for c in reversed(reads[i]))
    return write_fasta(dst, reads)


def long_insertion(path):
    """A 120-base reference and 6 reads: the reference, two reads with the
    same 600-base insertion at position 60 (longer than the 512-cell F window
    of the convex backtrack: the first of them walks it as one insertion, the
    second aligns along the new branch), two with an 1100-base insertion
    (a branch longer than the row ring, three windows long), the reference."""
    rng = random.Random(600)
    ref = "".join(rng.choice("ACGT") for _ in range(120))
    ins600 = "".join(rng.choice("ACGT") for _ in range(600))
    ins1100 = "".join(rng.choice("ACGT") for _ in range(1100))
    a = ref[:60] + ins600 + ref[60:]
    b = ref[:60] + ins1100 + ref[60:]
    return write_fasta(path, [ref, a, a, b, b, ref])


def amino(path, length=300, depth=10):
    rng = random.Random(5)
    aa = "ARNDCQEGHILKMFPSTWYV"
    ref = "".join(rng.choice(aa) for _ in range(length))
    reads = []
    for _ in range(depth):
        s = []
        for ch in ref:
            r = rng.random()
            if r < 0.04:
                s.append(rng.choice(aa))
            elif r < 0.07:
                pass
            elif r < 0.09:
                s.extend((ch, rng.choice(aa)))
            else:
                s.append(ch)
        reads.append("".join(s))
    return write_fasta(path, reads)


def fastq(path, length=400, depth=12, seed=31):
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(length))
    with open(path, "w") as f:
        for i in range(depth):
            out = []
            for ch in ref:
                r = rng.random()
                if r < 0.04:
                    out.append(rng.choice("ACGT"))
                elif r < 0.07:
                    pass
                else:
                    out.append(ch)
            s = "".join(out)
            qual = "".join(chr(33 + rng.randrange(5, 40)) for _ in s)
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, qual))
    return str(path)
