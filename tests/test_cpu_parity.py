"""CPU-side parity: host pipeline + scalar oracle DP vs the reference's
committed golden outputs, and (when the reference tree is present) vs the
live reference binary on fresh synthetic inputs.

These tests pin the oracle per SURVEY.md §8(c): every golden fixture the
reference's own regression suite checks, plus synthetic read sets at several
shapes. The oracle is injected explicitly (ABPOA_AMD_TEST_ALIGNER_SO); the
product GPU path is covered by tests/test_gpu_parity.py.
"""
import os
import subprocess
import pytest

from conftest import GOLDEN, ROOT, run_stdout
import seam_cases as sc

CASES = [
    ("seq.fa", [], "expected_seq_cons.txt"),
    ("seq.fa", ["-a1"], "expected_seq_msa.txt"),
    ("seq.fa", ["-r1"], "expected_seq_r1.txt"),
    ("seq.fa", ["-r2"], "expected_seq_r2.txt"),
    ("seq.fa", ["-m1"], "expected_seq_local.txt"),
    ("seq.fa", ["-m2"], "expected_seq_extend.txt"),
    ("seq.fa", ["-r3"], "expected_seq_gfa.txt"),
    ("seq.fa", ["-r5"], "expected_seq_fq.txt"),
    ("test.fa", [], "expected_test_cons.txt"),
    ("heter.fa", [], "expected_heter_cons.txt"),
    # path scores, gap placement, end bonus (tests/golden/make_golden.sh)
    ("seq.fa", ["-G", "-r1"], "expected_seq_G_r1.txt"),
    ("seq.fa", ["-R", "-r1"], "expected_seq_R_r1.txt"),
    ("seq.fa", ["-J", "-r1"], "expected_seq_J_r1.txt"),
    ("heter.fa", ["-R"], "expected_heter_R.txt"),
    ("seq.fa", ["-e", "5", "-m2"], "expected_seq_e5_extend.txt"),
    ("synth13_seed1.fa", ["-O", "4", "-E", "2", "-G", "-r1"], "expected_synth13_affine_G_r1.txt"),
    ("synth13_seed1.fa", ["-O", "0", "-E", "2", "-G", "-r1"], "expected_synth13_linear_G_r1.txt"),
]


@pytest.mark.parametrize("fa,opts,expected", CASES,
                         ids=["%s%s" % (c[0], "".join(c[1])) for c in CASES])
def test_golden(cputest_bin, oracle_env, fa, opts, expected):
    out = run_stdout([cputest_bin, os.path.join(GOLDEN, fa)] + opts, env=oracle_env)
    want = open(os.path.join(GOLDEN, expected), "rb").read()
    assert out == want


@pytest.mark.parametrize("seed,length,depth", [(1, 500, 20), (2, 1000, 30), (3, 2000, 10)])
def test_synthetic_vs_reference(cputest_bin, oracle_env, ref_bin, tmp_path, seed, length, depth):
    fa = tmp_path / "s.fa"
    subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), str(fa),
                    "--seed", str(seed), "--len", str(length), "--depth", str(depth)],
                   check=True, stderr=subprocess.DEVNULL)
    for opts in ([], ["-r1"]):
        ref = run_stdout([ref_bin, str(fa)] + opts)
        got = run_stdout([cputest_bin, str(fa)] + opts, env=oracle_env)
        assert got == ref, "divergence at seed=%d len=%d opts=%r" % (seed, length, opts)


# golden with the flag, golden of the same command without it
FLAG_GOLDENS = [
    ("expected_seq_G_r1.txt", "expected_seq_r1.txt"),
    ("expected_seq_R_r1.txt", "expected_seq_r1.txt"),
    ("expected_seq_J_r1.txt", "expected_seq_r1.txt"),
    ("expected_heter_R.txt", "expected_heter_cons.txt"),
]


@pytest.mark.parametrize("with_flag,without", FLAG_GOLDENS, ids=[c[0][9:-4] for c in FLAG_GOLDENS])
def test_flag_goldens_differ_from_plain(with_flag, without):
    """A flag's golden pins the flag only if the reference's output with it
    differs from its output without it on that input."""
    a = open(os.path.join(GOLDEN, with_flag), "rb").read()
    b = open(os.path.join(GOLDEN, without), "rb").read()
    assert a and b and a != b


@pytest.mark.parametrize("gap", [["-O", "4", "-E", "2"], ["-O", "0", "-E", "2"]], ids=["affine", "linear"])
def test_path_score_golden_differs_from_plain(cputest_bin, oracle_env, gap):
    """-G on the committed 13 % set changes the rows in affine and linear mode
    (affine -G changes nothing on seq.fa, heter.fa or test.fa)."""
    fa = os.path.join(GOLDEN, "synth13_seed1.fa")
    plain = run_stdout([cputest_bin, fa] + gap + ["-r1"], env=oracle_env)
    name = "expected_synth13_%s_G_r1.txt" % ("affine" if gap[1] == "4" else "linear")
    assert plain and plain != open(os.path.join(GOLDEN, name), "rb").read()


def test_end_bonus_is_parsed_and_never_read():
    """-e sets end_bonus, which neither the reference's aligner nor ours reads
    (abpoa_align_simd.c:1132 leaves it a TODO): the golden of -e 5 -m2 is the
    golden of -m2. There is no input on which -e has an effect to guard."""
    a = open(os.path.join(GOLDEN, "expected_seq_e5_extend.txt"), "rb").read()
    assert a and a == open(os.path.join(GOLDEN, "expected_seq_extend.txt"), "rb").read()


FLAG_CASES = [["-G"], ["-G", "-O", "4", "-E", "2"], ["-G", "-O", "0", "-E", "2"], ["-R"], ["-J"],
              ["-R", "-J", "-O", "4", "-E", "2"], ["-e", "5", "-m2"]]


@pytest.mark.parametrize("opts", FLAG_CASES, ids=lambda o: "".join(o))
def test_flags_vs_reference(cputest_bin, oracle_env, ref_bin, tmp_path, opts):
    """-G, -R, -J and -e against the live reference on a fresh 13 % set."""
    fa = sc.synth13(tmp_path / "s.fa")
    for extra in ([], ["-r1"]):
        ref = run_stdout([ref_bin, str(fa)] + opts + extra)
        got = run_stdout([cputest_bin, str(fa)] + opts + extra, env=oracle_env)
        assert ref and got == ref, "divergence opts=%r" % (opts + extra,)


# int16 scores with a large gap extension: inf_min = INT16_MIN + 1125 + 512 * 90
# = +14437, a "minus infinity" above every real score
POSITIVE_INF_MIN = ["-M", "90", "-X", "180", "-O", "180,1080", "-E", "90,45"]


@pytest.mark.parametrize("gap", [["-O", "180,1080", "-E", "90,45"], ["-O", "180", "-E", "90"],
                                 ["-O", "0", "-E", "90"]], ids=["convex", "affine", "linear"])
def test_positive_inf_min_is_refused(cputest_bin, oracle_env, gap):
    """The seam refuses the regime with one message, not a backtrack dead end."""
    p = subprocess.run([cputest_bin, os.path.join(GOLDEN, "seq.fa"), "-M", "90", "-X", "180"] + gap,
                       env=oracle_env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and p.stdout == b""
    import re
    m = re.search(rb"unsupported scoring: at int16 the out-of-band score floor is (\d+) \(>= 0\)", p.stderr)
    # INT16_MIN + max(min_mis, oe1, oe2) + 512 * 90
    assert m and int(m.group(1)) == -32768 + (1125 if gap[1] == "180,1080" else 270 if gap[1] == "180" else 180) + 46080
    assert b"dead end" not in p.stderr


def test_scaled_scoring_below_the_bound_is_not_refused(cputest_bin, oracle_env):
    """-M 60 at the same ratio keeps inf_min at -1298: same consensus as default."""
    out = run_stdout([cputest_bin, os.path.join(GOLDEN, "seq.fa"), "-M", "60", "-X", "120",
                      "-O", "120,720", "-E", "60,30"], env=oracle_env)
    assert out == open(os.path.join(GOLDEN, "expected_seq_cons.txt"), "rb").read()


@pytest.fixture(scope="module")
def width_bins(ref_bin):
    """The reference built twice at explicit ISAs (oracle/Makefile, `make
    widths`): (-msse4.1 build, -mavx512bw build). Skipped where they cannot be
    built, or where this CPU cannot run the AVX512 one."""
    bins = [os.path.join(os.path.dirname(ref_bin), n) for n in ("abpoa_sse41", "abpoa_avx512")]
    if not all(os.path.exists(b) for b in bins) and os.path.isdir("/root/reference"):
        subprocess.run(["make", "-j4", "widths"], cwd=os.path.join(ROOT, "oracle"),
                       check=True, stdout=subprocess.DEVNULL)
    if not all(os.path.exists(b) for b in bins):
        pytest.skip("explicit-ISA reference builds unavailable")
    if "avx512bw" not in open("/proc/cpuinfo").read():
        pytest.skip("this CPU cannot run the AVX512 build")
    return bins


def test_positive_inf_min_reference_depends_on_vector_width(width_bins, tmp_path):
    """Why that regime is refused and not reproduced: on this input the
    reference built with -mavx512bw (32 int16 lanes) errors out of
    cg_backtrack while the same sources built with -msse4.1 (8 lanes) print
    rows. (An -mavx2 build, 16 lanes, agreed with SSE4.1 when tried.)"""
    fa = sc.synth13(tmp_path / "s.fa", seed=105, length=60, depth=10)
    runs = [subprocess.run([b, fa] + POSITIVE_INF_MIN + ["-r1"], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL) for b in width_bins]
    assert runs[0].returncode == 0 and runs[0].stdout
    assert (runs[0].returncode, runs[0].stdout) != (runs[1].returncode, runs[1].stdout)


def test_product_fails_loudly_without_aligner(cputest_bin):
    """The CPU test binary must refuse to align without an injected oracle
    (mirrors the product's no-silent-fallback guarantee)."""
    p = subprocess.run([cputest_bin, os.path.join(GOLDEN, "seq.fa")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0
    assert b"no GPU aligner" in p.stderr or b"CPU-only TEST build" in p.stderr


MODE_CASES = [
    ["-O", "4", "-E", "2"],          # affine
    ["-O", "0", "-E", "2"],          # linear
    ["-m1"],                          # local (convex)
    ["-m2"],                          # extension (convex)
    ["-O", "4", "-E", "2", "-m1"],   # local affine
    ["-O", "0", "-E", "2", "-m2"],   # extension linear
]


@pytest.mark.parametrize("opts", MODE_CASES, ids=lambda o: "".join(o))
def test_modes_vs_reference(cputest_bin, oracle_env, ref_bin, tmp_path, opts):
    fa = tmp_path / "s.fa"
    subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), str(fa),
                    "--seed", "7", "--len", "1200", "--depth", "25"],
                   check=True, stderr=subprocess.DEVNULL)
    ref = run_stdout([ref_bin, str(fa)] + opts)
    got = run_stdout([cputest_bin, str(fa)] + opts, env=oracle_env)
    assert got == ref


def test_aa_mode_vs_reference(cputest_bin, oracle_env, ref_bin, tmp_path):
    """Amino-acid alphabet (m=27) with BLOSUM62, global affine (configs[3])."""
    import random
    random.seed(5)
    aa = "ARNDCQEGHILKMFPSTWYV"
    refseq = "".join(random.choice(aa) for _ in range(400))
    reads = []
    for _ in range(10):
        s = []
        for ch in refseq:
            r = random.random()
            if r < 0.04: s.append(random.choice(aa))
            elif r < 0.07: pass
            elif r < 0.09: s.extend((ch, random.choice(aa)))
            else: s.append(ch)
        reads.append("".join(s))
    fa = tmp_path / "aa.fa"
    with open(fa, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    mtx = os.path.join(GOLDEN, "BLOSUM62.mtx")
    for opts in (["-c", "-t", mtx, "-O", "4", "-E", "2"], ["-c", "-t", mtx]):
        ref = run_stdout([ref_bin, str(fa)] + opts)
        got = run_stdout([cputest_bin, str(fa)] + opts, env=oracle_env)
        assert got == ref


def test_pog_dot_output(cputest_bin, oracle_env, ref_bin, tmp_path):
    """--out-pog DOT file is byte-identical to the reference's (the graphviz
    render step itself needs `dot`, absent here; both sides fail alike)."""
    import subprocess
    ref_png = tmp_path / "ref.png"
    amd_png = tmp_path / "amd.png"
    fa = os.path.join(GOLDEN, "seq.fa")
    subprocess.run([ref_bin, fa, "-g", str(ref_png)], stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    subprocess.run([cputest_bin, fa, "-g", str(amd_png)], env=oracle_env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ref_dot = open(str(ref_png) + ".dot", "rb").read()
    amd_dot = open(str(amd_png) + ".dot", "rb").read()
    assert ref_dot == amd_dot


def test_list_input_mode(cputest_bin, oracle_env, ref_bin, tmp_path):
    """-l: input file is a list of FASTA paths, one MSA per file with
    batch_index-numbered consensus headers (abpoa.c:152-161)."""
    lst = tmp_path / "list.txt"
    fas = []
    for seed in (61, 62):
        fa = tmp_path / ("s%d.fa" % seed)
        subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), str(fa),
                        "--seed", str(seed), "--len", "400", "--depth", "8"],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        fas.append(str(fa))
    lst.write_text("".join(p + "\n" for p in fas))
    for opts in ([], ["-r1"]):
        ref = subprocess.run([ref_bin, "-l", str(lst)] + opts, stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL).stdout
        amd = run_stdout([cputest_bin, "-l", str(lst)] + opts, env=oracle_env)
        assert ref == amd


def test_quality_weights_fastq(cputest_bin, oracle_env, ref_bin, tmp_path):
    """-Q: FASTQ qualities become per-base edge weights; weighted consensus,
    MSA, FASTQ output and weighted multi-consensus must match."""
    import random
    rng = random.Random(31)
    ref_seq = "".join(rng.choice("ACGT") for _ in range(500))
    fq = tmp_path / "q.fq"
    with open(fq, "w") as f:
        for i in range(12):
            out = []
            for ch in ref_seq:
                r = rng.random()
                if r < 0.04: out.append(rng.choice("ACGT"))
                elif r < 0.07: pass
                else: out.append(ch)
            s = "".join(out)
            qual = "".join(chr(33 + rng.randrange(5, 40)) for _ in s)
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, qual))
    for opts in (["-Q"], ["-Q", "-r1"], ["-Q", "-d2"], ["-Q", "-r4"], ["-Q", "-a1"]):
        ref = subprocess.run([ref_bin, str(fq)] + opts, stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL).stdout
        amd = run_stdout([cputest_bin, str(fq)] + opts, env=oracle_env)
        assert ref == amd, "mismatch opts=%r" % (opts,)
