#!/bin/bash
# Regenerates the golden parity fixtures committed under tests/golden/.
#
# Inputs are the reference's own test data (test data, not code) copied from
# /root/reference/test_data; expected outputs are produced by the reference
# binary built by oracle/Makefile from the reference's unmodified sources.
# /root/reference exists only in the dev container, so the fixtures are
# committed and the GPU-side tests read them from here.
#
# Usage: bash tests/golden/make_golden.sh   (from anywhere)
set -e
cd "$(dirname "$0")"
REF=/root/reference
BIN=../../oracle/_ref/abpoa
[ -x "$BIN" ] || { echo "build oracle/_ref first: (cd oracle && make)"; exit 1; }

for f in seq.fa heter.fa 3alleles.fa test.fa; do
    cp "$REF/test_data/$f" .
done

run() { # run <outfile> <args...>
    out=$1; shift
    "$BIN" "$@" 2>/dev/null > "$out"
}

# the three upstream regression goldens (tests/run_all.sh:33-56 in the reference)
run expected_seq_cons.txt       seq.fa
run expected_seq_msa.txt        seq.fa -a1
run expected_heter_d2.txt       heter.fa -d2
# extra configurations covering the north-star variants on the small input
run expected_seq_r1.txt         seq.fa -r1          # RC-MSA output
run expected_seq_r2.txt         seq.fa -r2          # cons + MSA
run expected_seq_affine.txt     seq.fa -O 4 -E 2    # affine gap
run expected_seq_linear.txt     seq.fa -O 0 -E 2    # linear gap
run expected_seq_local.txt      seq.fa -m 1         # local mode
run expected_seq_extend.txt     seq.fa -m 2         # extension mode
run expected_seq_gfa.txt        seq.fa -r3          # GFA output
run expected_seq_fq.txt         seq.fa -r5          # FASTQ consensus
run expected_test_cons.txt      test.fa
run expected_3alleles_d3.txt    3alleles.fa -d3
run expected_heter_cons.txt     heter.fa
# flags that no GPU test ran before the seam harness: path scores, gap
# placement, end bonus. Each is committed on an input on which the flag changes
# this binary's output (tests/test_cpu_parity.py guards that), except -e, which
# the reference parses and never reads: its golden equals expected_seq_extend.txt.
run expected_seq_G_r1.txt       seq.fa -G -r1
run expected_seq_R_r1.txt       seq.fa -R -r1
run expected_seq_J_r1.txt       seq.fa -J -r1
run expected_heter_R.txt        heter.fa -R
run expected_seq_e5_extend.txt  seq.fa -e 5 -m2
# affine -G changes nothing on the four inputs above; seed 1 is the first
# 400 x 24 set at 13 % error on which it does (and linear -G as well)
python3 ../make_synth.py synth13_seed1.fa --seed 1 --len 400 --depth 24 \
    --sub 0.06 --del 0.04 --ins 0.03 2>/dev/null
run expected_synth13_affine_G_r1.txt synth13_seed1.fa -O 4 -E 2 -G -r1
run expected_synth13_linear_G_r1.txt synth13_seed1.fa -O 0 -E 2 -G -r1
echo "golden fixtures regenerated"
