"""Two-stage flat row-column MSA (the device MSA kernels' shared body) vs
abpoa_generate_rc_msa on the pointer graph, on CPU.

abpoa_amd_msatwin replays oracle CIGARs into the pointer graph and the flat
device-layout graph and, after EVERY read, runs abamd_flat_msa_rank_cols and
abamd_flat_msa_place (one lane) over the flat graph, with the phased flat
consensus supplying the consensus row as on the device, and compares msa_len
and every row byte against abpoa_generate_rc_msa — with and without the
consensus row — and once more through abamd_cons_attach_msa."""
import os
import subprocess

import cons_cases
from conftest import ROOT, CSRC, GOLDEN, ORACLE_SO

TWIN = os.path.join(CSRC, "abpoa_amd_msatwin")


def _run(fa):
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    out = subprocess.run([TWIN, fa], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, "%s: %s" % (fa, out.stderr.decode()[-500:])
    assert b"msa twin OK" in out.stdout
    return out.stdout.decode()


def test_msa_twin_golden(cputest_bin):
    # 3alleles.fa has a three-member aligned group in one column
    for fa in ("seq.fa", "test.fa", "heter.fa", "3alleles.fa"):
        _run(os.path.join(GOLDEN, fa))


def test_msa_twin_synthetic(cputest_bin, tmp_path):
    # the shapes of test_cons_twin.py::test_cons_twin_synthetic; depth 80
    # gives two read-id bitset words
    for seed, length, depth in ((1, 300, 12), (2, 900, 20), (3, 1800, 30), (4, 4000, 40),
                                (5, 600, 80)):
        fa = str(tmp_path / ("s%d.fa" % seed))
        subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), fa,
                        "--seed", str(seed), "--len", str(length), "--depth", str(depth)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = _run(fa)
        assert ("%d words" % (1 + (depth - 1) // 64)) in out


def test_msa_twin_tie_stress(cputest_bin, tmp_path):
    """SNP columns (two-member aligned groups), a 3-base deletion, and row
    counts around 64."""
    for name, reads in cons_cases.all_sets():
        fa = str(tmp_path / (name + ".fa"))
        cons_cases.write_fasta(fa, reads)
        _run(fa)
