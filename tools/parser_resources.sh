#!/bin/bash
# Measurement build (here, no GPU needed): the compiler's view of the slice parser. Compiles csrc/rbt_kernels_parse.hip with the Makefile's flags twice - as the product
# (both instantiations of rbt_parse_slice behind one branch) and with -DRBT_PARSE_INTRA_ONLY (csrc/rbt_parse.h: the intra-only instantiation alone; never the product) -
# and prints, for k_parse_tasks<384>, what -Rpass-analysis=kernel-resource-usage reports plus the instruction count of the kernel's assembly.
# The figures of a run are kept in profiles/r05_parser_resources.txt.
cd "$(dirname "$0")/../rabbit-transcoding_amd" || exit 1
T=$(mktemp -d) || exit 1
FLAGS="--offload-arch=gfx950 -std=c++17 -O3 -fPIC -Wall -Wno-unused-function --cuda-device-only -S -Rpass-analysis=kernel-resource-usage"
one() {   # $1 = label, $2.. = extra flags
  local label=$1; shift
  /opt/rocm/bin/hipcc $FLAGS "$@" csrc/rbt_kernels_parse.hip -o $T/$label.s 2> $T/$label.log || { tail -5 $T/$label.log; exit 1; }
  echo "== $label"
  grep -A12 'Function Name: _ZN4rbtk13k_parse_tasksILi384' $T/$label.log | grep -E 'TotalSGPRs|VGPRs:|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill' | sed 's/.*remark: *//; s/ \[-Rpass.*//'
  # instructions between the kernel's label and its end (lines that start with a tab and a mnemonic, no directives, labels or comments)
  awk '/^_ZN4rbtk13k_parse_tasksILi384[^:]*:/{f=1; next} f && /^\.Lfunc_end/{exit} f && /^\t[a-z]/{n++} END{print "Instructions: " n}' $T/$label.s
}
one product &
one intra_only -DRBT_PARSE_INTRA_ONLY &
wait
rm -rf $T
