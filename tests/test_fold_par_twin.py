"""Lane-parallel graph mutation walk (abamd_fold_par.inc) vs the serial walk.

abpoa_amd_foldpartwin feeds the same oracle CIGARs to three flat graphs: the
serial abamd_flat_apply_alignment, the phased walk with one lane, and the
phased walk with 64 lanes emulated on the host (a lane loop inside each phase,
prefix sums through the same per-lane arrays the device uses). After every
read both phased graphs must equal the serial one in every field — pools up to
their counts, chain heads and tails, read-id words, n_read, n_span_read, the
qpos map and the four counters — and no fold may take the serial fallback:
its guards cover invariant violations only, which valid alignments never
produce."""
import os
import random
import re
import subprocess

from conftest import ROOT, GOLDEN, ORACLE_SO

TWIN = os.path.join(ROOT, "abpoa_amd", "csrc", "abpoa_amd_foldpartwin")
OK_RE = re.compile(rb"partwin OK \((\d+) reads, .* fallbacks (\d+), partition differs (\d+)\)")
READ_RE = re.compile(r"read (\d+) n_cigar (\d+) max_ins (\d+) first_ins (\d+) last_ins (\d+) "
                     r"new_nodes (\d+) new_edges (\d+)")


def _run(fa, extra=()):
    """Run the twin; returns (partition_differs, per-read dicts when -v)."""
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    out = subprocess.run([TWIN, fa] + list(extra), env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-500:]
    m = OK_RE.search(out.stdout)
    assert m, out.stdout.decode()[-500:]
    assert int(m.group(2)) == 0
    keys = ("read", "n_cigar", "max_ins", "first_ins", "last_ins", "new_nodes", "new_edges")
    reads = [dict(zip(keys, map(int, r))) for r in READ_RE.findall(out.stdout.decode())]
    return int(m.group(3)), reads


def _both(fa):
    d0, reads = _run(fa, ["-v"])
    d1, _ = _run(fa, ["-r1"])
    return d0 and d1, reads


def test_golden():
    # seq.fa reads have far more than 64 ops: lane 0 of 64 owns a strict part
    # of the CIGAR, so the intermediate state differs from the 1-lane walk
    differs, _ = _both(os.path.join(GOLDEN, "seq.fa"))
    assert differs
    _both(os.path.join(GOLDEN, "fgt.fa"))


def test_synthetic(tmp_path):
    # 900 x 20 grows aligned groups of 3+ members; depth 80 needs two read-id
    # words per edge (rid_n = 2)
    for seed, length, depth in ((1, 300, 12), (2, 900, 20), (5, 600, 80)):
        fa = str(tmp_path / ("s%d.fa" % seed))
        subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), fa,
                        "--seed", str(seed), "--len", str(length), "--depth", str(depth)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        differs, _ = _both(fa)
        assert differs


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _write(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    return str(path)


def test_handmade(tmp_path):
    rng = random.Random(7)

    # fewer ops than lanes: most lanes own nothing
    b = _rand(rng, 40)
    sub = b[:17] + ("A" if b[17] != "A" else "C") + b[18:]
    _, reads = _both(_write(tmp_path / "short.fa", [b, sub, b[:30], sub]))
    assert all(r["n_cigar"] < 64 for r in reads[1:])

    # exactly one op per lane, and one more than that
    for n in (64, 65):
        b = _rand(rng, n)
        _, reads = _both(_write(tmp_path / ("ops%d.fa" % n), [b, b, b]))
        assert [r["n_cigar"] for r in reads[1:]] == [n, n]
        # a read identical to the backbone adds no node and no edge
        assert all(r["new_nodes"] == 0 and r["new_edges"] == 0 for r in reads[1:])

    # an insertion run longer than 64 bases, starting before op 64 and ending
    # after it; later reads walk the inserted nodes as existing ones
    b = _rand(rng, 140)
    ins = _rand(rng, 90)
    long_ins = b[:60] + ins + b[60:]
    _, reads = _both(_write(tmp_path / "longins.fa", [b, long_ins, b, long_ins]))
    assert reads[1]["max_ins"] > 64 and reads[1]["new_nodes"] > 64, reads[1]

    # insertion at the first query base, and at the last
    b = _rand(rng, 100)
    first = _rand(rng, 6) + b
    last = b + _rand(rng, 6)
    _, reads = _both(_write(tmp_path / "ends.fa", [b, first, last, first, last, b]))
    assert reads[1]["first_ins"] > 0, reads[1]
    assert reads[2]["last_ins"] > 0, reads[2]


def test_guards_leave_graph_untouched():
    """Corrupted CIGARs (a node visited twice, an id beyond the pool, an
    insertion longer than the read) trip the guards with 1 and with 64 lanes,
    and the graph stays exactly as it was."""
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    out = subprocess.run([TWIN, os.path.join(GOLDEN, "seq.fa"), "-r1", "-g"], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-500:]
    assert b"guards OK" in out.stdout and OK_RE.search(out.stdout)
