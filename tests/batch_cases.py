"""Inputs and option sets shared by tests/test_resident_paths_gpu.py (the
device-resident batch driver against the oracle on every workload and recovery
path), tests/test_batch_flags_cpu.py (the batch harness parses like the CLI)
and tests/test_arena_overflow_cpu.py (the overflow inputs do overflow).

Every generator is deterministic and writes one FASTA per read set."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_synth  # noqa: E402
import seam_cases as sc  # noqa: E402

BLOSUM = sc.BLOSUM
AA = "ARNDCQEGHILKMFPSTWYV"

# ---- (a) the ragged batch --------------------------------------------------
# depth 1 and 2 run out of reads after round 0 / 1 (their items empty early);
# the 20 x 400 set is the deep-short shape whose graph gets far predecessors
RAGGED = [(1, 80), (2, 300), (3, 300), (7, 700), (12, 1100), (20, 1500), (20, 400)]


def _write(path, reads):
    return sc.write_fasta(path, reads)


def ragged(dirpath):
    """7 sets, make_synth.py's 10 % error model (4.5 % sub / 3 % del / 2.5 % ins)."""
    rng = random.Random(20240)
    paths = []
    for i, (depth, length) in enumerate(RAGGED):
        _ref, reads = make_synth.gen_set(rng, depth, length, 0.045, 0.03, 0.025)
        paths.append(_write(os.path.join(str(dirpath), "rag%d_d%d_l%d.fa" % (i, depth, length)), reads))
    return paths


def ragged_lengths():
    return [length for _d, length in RAGGED]


AFFINE = ["-O", "4", "-E", "2"]
LINEAR = ["-O", "0", "-E", "2"]
GAPS = {"convex": [], "affine": AFFINE, "linear": LINEAR}

# (id, options, predicate on the set's reference length)
WORKLOADS = []
for _g in sc.GAP_IDS:
    WORKLOADS.append((_g, GAPS[_g], None))
    WORKLOADS.append((_g + "-local", GAPS[_g] + ["-m1"], None))
    WORKLOADS.append((_g + "-extend", GAPS[_g] + ["-m2"], None))
    WORKLOADS.append((_g + "-extend-z5", GAPS[_g] + ["-m2", "-z", "5"], None))
for _g in ("convex", "affine"):
    WORKLOADS.append((_g + "-b241", GAPS[_g] + ["-b", "241"], None))
    # unbanded: every row is qlen + 1 cells wide; the long sets are left out
    WORKLOADS.append((_g + "-unbanded", GAPS[_g] + ["-b", "-1"], lambda n: n <= 700))
WORKLOADS.append(("convex-M9", ["-M", "9"], None))
for _g in sc.GAP_IDS:
    # default scoring x45: int32 from 400 bases on; shorter sets are refused by
    # design at int16 and stay out
    WORKLOADS.append((_g + "-x45", sc.GAPS_X45[_g], lambda n: n >= 400))
WORKLOAD_IDS = [w[0] for w in WORKLOADS]


def workload_files(paths, keep):
    if keep is None:
        return list(paths)
    return [p for p, n in zip(paths, ragged_lengths()) if keep(n)]


# ---- (b) amino acids -------------------------------------------------------
AA_OPTS = ["-c", "-t", BLOSUM, "-O", "4", "-E", "2"]  # as bench.py sets its aa workload


def amino(dirpath):
    """3 sets x 6 reads, 150 / 270 / 400 residues, alphabet 20."""
    rng = random.Random(62)
    paths = []
    for i, length in enumerate((150, 270, 400)):
        ref = "".join(rng.choice(AA) for _ in range(length))
        reads = []
        for _ in range(6):
            s = []
            for ch in ref:
                r = rng.random()
                if r < 0.05:
                    s.append(rng.choice(AA))
                elif r < 0.08:
                    pass
                elif r < 0.10:
                    s.extend((ch, rng.choice(AA)))
                else:
                    s.append(ch)
            reads.append("".join(s))
        paths.append(_write(os.path.join(str(dirpath), "aa%d.fa" % i), reads))
    return paths


# ---- (c) mixed widths ------------------------------------------------------
MIXED_OPTS = ["-M", "30", "-X", "60", "-O", "60,360", "-E", "30,15"]


def mixed(dirpath):
    """The three sets of test_seam_gpu.test_mixed_width_batch: 300 and 700
    bases pick int16 (the 700 set until its graph passes 1072 rows), 1300 picks
    int32."""
    return [sc.synth(os.path.join(str(dirpath), "mix%d.fa" % n), n, n, 8, rates=None)
            for n in (300, 700, 1300)]


# ---- (d) DP arena overflow -------------------------------------------------
# The drivers reserve rows * (2w + 160) + qlen + 64 cells per job. A long
# insertion near the 3' end that the graph carries and the read lacks makes
# every row before the bubble as wide as the insertion (the band's lower edge
# follows qlen - max_remain, and max_remain counts the insertion), and the rows
# of the bubble itself as wide as what is left of it.
D_SPEC = {
    # name: (reference length, insertion length, insertion position, reads with, reads without)
    "D1": (1200, 400, 1000, 2, 3),
    "D2": (800, 1200, 700, 2, 3),
}


def overflow_set(dirpath, name):
    ref_l, ins_l, pos, n_with, n_without = D_SPEC[name]
    rng = random.Random(hash_name(name))
    ref = "".join(rng.choice("ACGT") for _ in range(ref_l))
    ins = "".join(rng.choice("ACGT") for _ in range(ins_l))
    carrier = ref[:pos] + ins + ref[pos:]
    light = (0.01, 0.005, 0.005)  # enough to branch the graph, not to hide the bubble
    reads = [make_synth.mutate(rng, carrier, *light) for _ in range(n_with)]
    reads += [make_synth.mutate(rng, ref, *light) for _ in range(n_without)]
    return _write(os.path.join(str(dirpath), "%s.fa" % name), reads)


def hash_name(name):
    return {"D1": 1001, "D2": 1002}[name]


def overflow_batch(dirpath):
    """D1, D2 and two ordinary sets (the ragged batch's 7 x 700 and 3 x 300)."""
    rag = ragged(dirpath)
    return [overflow_set(dirpath, "D1"), rag[3], overflow_set(dirpath, "D2"), rag[2]]


# ---- (f) a read that aligns nowhere -----------------------------------------
# The candidate for an empty CIGAR. It does not give one (no
# input can): the backtrack reports the whole read as one insertion.
UNALIGNED_OPTS = ["-m1"]


def unaligned_set(dirpath):
    """Local mode: three reads over C/G/T, a poly-A read that scores 0 against
    every node, two more ordinary reads."""
    rng = random.Random(7)
    ref = "".join(rng.choice("CGT") for _ in range(200))

    def mut():
        return "".join(c if rng.random() > 0.04 else rng.choice("CGT") for c in ref)
    reads = [mut(), mut(), mut(), "A" * 120, mut(), mut()]
    return _write(os.path.join(str(dirpath), "unaligned.fa"), reads)


# ---- running the harness and the oracle ------------------------------------
def records(out):
    """[(consensus, [msa rows])] per ">set_N" record of the batch harness."""
    recs = []
    for rec in out.decode().split(">")[1:]:
        lines = rec.split("\n")
        assert lines[0].startswith("set_") and lines[-1] == ""
        recs.append((lines[1], lines[2:-1]))
    return recs


def parse_stats(stderr):
    """The harness's -S line as a dict of ints."""
    lines = [ln for ln in stderr.decode().splitlines() if ln.startswith("[batch-stats] ")]
    assert len(lines) == 1, stderr.decode()[-2000:]
    return {k: int(v) for k, v in (kv.split("=") for kv in lines[0].split()[1:])}


_EXPECTED = {}


def oracle_rows(cputest_bin, oracle_env, opts, fa):
    """The expected output for one set: the sequence lines of the sequential
    CPU CLI with the oracle injected, `opts -r2` (read rows, then the consensus
    row). Computed once per (options, file) and shared."""
    import subprocess
    key = (tuple(opts), fa)
    if key not in _EXPECTED:
        out = subprocess.run([cputest_bin] + list(opts) + ["-r2", fa], env=oracle_env, check=True,
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
        rows = [ln for ln in out.splitlines() if not ln.startswith(">")]
        assert rows
        _EXPECTED[key] = rows
    return _EXPECTED[key]


def check_against_oracle(recs, cputest_bin, oracle_env, opts, files):
    """Every record of a `-r2` harness run equals the oracle's output for its
    set: all read rows, the consensus row, and the consensus record."""
    assert len(recs) == len(files)
    for i, fa in enumerate(files):
        want = oracle_rows(cputest_bin, oracle_env, opts, fa)
        cons, rows = recs[i]
        assert rows == want, "set %d (%s): MSA rows differ from the oracle's" % (i, os.path.basename(fa))
        assert cons == want[-1].replace("-", ""), "set %d: consensus record differs" % i
