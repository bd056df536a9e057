#!/bin/bash
# Device-code identity of two builds of one csrc/*.hip file (attn.hip, gemm.hip, ...):  tools/device_diff.sh OLD/x.o NEW/x.o
# Extracts the gfx950 code object of each, compares the bytes and, kernel by kernel (symbols sorted by name, so an order
# change in the object does not count), the disassembly.  Exit 0: every kernel's instructions are identical.
set -euo pipefail
ROCM=${ROCM_PATH:-/opt/rocm}
BUNDLER=$ROCM/llvm/bin/clang-offload-bundler
OBJDUMP=$ROCM/llvm/bin/llvm-objdump
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
i=0
for o in "$1" "$2"; do
  i=$((i + 1))
  # the host object carries the offload bundle in its .hip_fatbin section
  $ROCM/llvm/bin/llvm-objcopy --dump-section .hip_fatbin="$T/$i.fatbin" "$o"
  $BUNDLER --unbundle --type=o --input="$T/$i.fatbin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$T/$i.co"
  sha256sum "$T/$i.co" | cut -d' ' -f1 > "$T/$i.sha"
  # one file per function symbol: its instructions and their encodings, without the addresses they happen to sit at
  $OBJDUMP -d --no-leading-addr "$T/$i.co" | sed -E 's#// [0-9A-F]+:#//#' |
    awk -v d="$T/$i.d" 'BEGIN { system("mkdir -p " d) } /^<.*>:$/ { f = d "/" substr($0, 2, length($0) - 3); next }
                        /^[ \t]*(\.\.\.)?$/ { next }      # zero fill between sections
                        f { print > f }'
  ls "$T/$i.d" | sort > "$T/$i.names"
done
echo "code object sha256: $(cat "$T/1.sha") / $(cat "$T/2.sha")"
if cmp -s "$T/1.co" "$T/2.co"; then echo "code objects byte-equal"; fi
diff "$T/1.names" "$T/2.names" > /dev/null || { echo "kernel sets differ"; diff "$T/1.names" "$T/2.names" | head; exit 1; }
n=0; bad=0
while read -r k; do
  n=$((n + 1))
  cmp -s "$T/1.d/$k" "$T/2.d/$k" || { echo "DIFFERS: $k"; bad=$((bad + 1)); }
done < "$T/1.names"
echo "$n functions compared, $bad differ"
[ "$bad" = 0 ]
