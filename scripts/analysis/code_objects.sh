#!/bin/sh
# Device code of two builds compared without a GPU: the gfx950 code objects of
# libhge.so, hge_batch.o and hge_verify.o are unbundled from both build directories and
# their .text bytes hashed.  A code object that differs gets its kernels' resource
# usage (.vgpr_count and the like from the metadata notes) diffed as well, and its
# functions are compared one by one over their instruction words: the ones that differ
# are listed by name.
#   scripts/analysis/code_objects.sh PARENT_BUILD_DIR BUILD_DIR > profiles/.../code_objects.txt
set -eu
A=$1
B=$2
LLVM=${LLVM:-/opt/rocm/llvm/bin}
TRIPLE=hipv4-amdgcn-amd-amdhsa--gfx950
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
# funcs CODE_OBJECT: one line per function, "name words", the words its instructions encode to
funcs() {
  "$LLVM/llvm-objdump" -d "$1" | awk '
    /^[0-9a-f]* *<.*>:$/ { if (name != "") print name, w; name = $0; sub(/^[^<]*</, "", name); sub(/>:$/, "", name); w = ""; next }
    name != "" && match($0, /\/\/ [0-9A-F]+: /) { x = substr($0, RSTART + RLENGTH); sub(/ <.*$/, "", x); gsub(/ /, "", x); w = w x }
    END { if (name != "") print name, w }' | sort -k1,1
}
rc=0
for f in libhge.so hge_batch.o hge_verify.o; do
  for side in a b; do
    [ $side = a ] && d=$A || d=$B
    "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$d/$f" "$T/$side.fatbin"
    "$LLVM/clang-offload-bundler" --type=o --unbundle --input="$T/$side.fatbin" --targets=$TRIPLE \
      --output="$T/$side.co"
    "$LLVM/llvm-objcopy" -O binary --only-section=.text "$T/$side.co" "$T/$side.text"
    "$LLVM/llvm-readelf" --notes "$T/$side.co" |
      grep -E '^ +\.(name|vgpr_count|agpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):' \
        > "$T/$side.res" || true
  done
  ha=$(sha256sum < "$T/a.text" | cut -d' ' -f1)
  hb=$(sha256sum < "$T/b.text" | cut -d' ' -f1)
  printf '%s gfx950 .text: parent %s bytes sha256 %s\n' "$f" "$(wc -c < "$T/a.text")" "$ha"
  printf '%s gfx950 .text: change %s bytes sha256 %s\n' "$f" "$(wc -c < "$T/b.text")" "$hb"
  if [ "$ha" = "$hb" ]; then
    printf '%s: identical (%s kernels)\n' "$f" "$(grep -c '\.name:' "$T/b.res")"
  else
    printf '%s: DIFFERENT; resource usage, parent (<) against change (>):\n' "$f"
    diff "$T/a.res" "$T/b.res" || true
    funcs "$T/a.co" > "$T/a.fn"
    funcs "$T/b.co" > "$T/b.fn"
    printf '%s: functions whose instruction words differ (bytes parent -> change):\n' "$f"
    join -a1 -a2 -e none -o 0,1.2,2.2 "$T/a.fn" "$T/b.fn" | awk '
      $2 != $3 { printf "  %s: %s -> %s\n", $1, $2 == "none" ? "absent" : length($2) / 2, $3 == "none" ? "absent" : length($3) / 2; d++ }
      $2 == $3 { s++ }
      END { printf "  %d functions differ, %d are identical word for word\n", d, s }'
    rc=1
  fi
done
exit $rc
