#!/bin/bash
# Compares the gfx950 device code of the eight step objects of two builds: compare_step_objects.sh OBJ_DIR_A OBJ_DIR_B [WORK_DIR].
# Per object: the offload bundle is taken out of .hip_fatbin and unbundled, and the code object's .text bytes and its
# disassembly are compared.  (The code objects as whole files differ between two build directories: the compilation-unit id
# in their symbol names is a hash that includes the source path.)  Exit status 1 if any .text differs.
set -euo pipefail
A="$1"; B="$2"; W="${3:-$(mktemp -d)}"
LLVM="${LLVM_BIN:-/opt/rocm/lib/llvm/bin}"
mkdir -p "$W"
bad=0
for b in 64 256 512 1024; do
    for p in 0 1; do
        n="step_${b}_${p}"
        for side in A B; do
            dir="$A"; [ "$side" = B ] && dir="$B"
            "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$W/$n.$side.fatbin" "$dir/$n.o"
            "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
                --input="$W/$n.$side.fatbin" --output="$W/$n.$side.co"
            "$LLVM/llvm-objcopy" -O binary --only-section=.text "$W/$n.$side.co" "$W/$n.$side.text"
            "$LLVM/llvm-objdump" -d --no-show-raw-insn "$W/$n.$side.co" | sed -E 's/^ *[0-9a-f]+://; /file format/d; s/<[^>]*>//g' > "$W/$n.$side.s"
        done
        text=identical; cmp -s "$W/$n.A.text" "$W/$n.B.text" || { text=DIFFERENT; bad=1; }
        asm=identical; cmp -s "$W/$n.A.s" "$W/$n.B.s" || asm=DIFFERENT
        echo "$n: .text $(stat -c %s "$W/$n.A.text") / $(stat -c %s "$W/$n.B.text") bytes $text, sha256 $(sha256sum "$W/$n.B.text" | cut -c1-16); disassembly ($(wc -l < "$W/$n.B.s") lines, symbol names dropped) $asm"
    done
done
exit $bad
