#!/bin/bash
# Device assembly of every csrc/*.hip at <git-rev> against the working tree (no GPU needed): per file, the number of
# differing lines; exit status 1 if any file differs.  The check for a kernel refactor that must not change the code.
# Each tree is compiled with the FLAGS= line of its own build.sh.
# usage: tools/device_asm_diff.sh <git-rev>
set -eu
[ $# -eq 1 ] || { echo "usage: $0 <git-rev>" >&2; exit 2; }
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=pti_ldm_vae_amd/csrc
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old" "$tmp/asm_old" "$tmp/asm_new"
git -C "$root" archive "$1" -- "$csrc" include | tar -x -C "$tmp/old"

emit() {   # emit <tree> <out dir>: one .s per .hip, without the __hip_cuid_ lines (a hash of the source text)
  local FLAGS f
  eval "$(grep '^FLAGS=' "$1/$csrc/build.sh")"
  for f in "$1/$csrc"/*.hip; do
    (cd "$1/$csrc" && hipcc $FLAGS -x hip --cuda-device-only -S "$(basename "$f")" -o -) | grep -v __hip_cuid_ \
      > "$2/$(basename "$f" .hip).s"
  done
}
emit "$tmp/old" "$tmp/asm_old"
emit "$root" "$tmp/asm_new"

status=0
for name in $(cd "$tmp" && ls asm_old asm_new | grep '\.s$' | sort -u); do
  if [ ! -f "$tmp/asm_old/$name" ] || [ ! -f "$tmp/asm_new/$name" ]; then
    echo "${name%.s}.hip: only in one tree"; status=1; continue
  fi
  n=$(diff "$tmp/asm_old/$name" "$tmp/asm_new/$name" | grep -c '^[<>]' || true)
  echo "${name%.s}.hip: $n"
  [ "$n" -eq 0 ] || status=1
done
exit $status
