#!/bin/bash
# Device assembly of every csrc/*.hip at <git-rev> against the working tree, compared PER KERNEL (no GPU needed).  Each
# file's assembly is split at the function symbols; a function's piece runs from its label to the next function and so
# holds its instructions, its .amdhsa_kernel descriptor (registers, LDS, scratch) and its resource summary.  Labels that
# are numbered by the function's index in the file (.LBB<n>_, BB<n>_ in comments, .Lfunc_end<n>, ...) and runs of white
# space are normalised, so removing one kernel does not make the ones after it differ.  Per file: the kernels that differ, those only in the old
# tree and those only in the new tree.  Exit status 0 exactly when no kernel present in both trees differs and none is
# new: the check for a refactor that must not change the code of the kernels it keeps.
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

emit() {   # emit <tree> <out dir>: one .s per .hip, eight compiles at a time
  local FLAGS f pids=() p
  eval "$(grep '^FLAGS=' "$1/$csrc/build.sh")"
  for f in "$1/$csrc"/*.hip; do
    (cd "$1/$csrc" && hipcc $FLAGS -x hip --cuda-device-only -S "$(basename "$f")" -o "$2/$(basename "$f" .hip).s") &
    pids+=($!)
    if [ ${#pids[@]} -eq 8 ]; then for p in "${pids[@]}"; do wait "$p"; done; pids=(); fi
  done
  for p in "${pids[@]}"; do wait "$p"; done
}
emit "$tmp/old" "$tmp/asm_old"
emit "$root" "$tmp/asm_new"

python3 -c "
import os, re, subprocess, sys
old_dir, new_dir = sys.argv[1:3]
begin = re.compile(r'; -- Begin function (\S+)')
lead = re.compile(r'\s*\.(section\s+\.text|text\b|protected|hidden|weak|globl)')          # a function's own preamble
tail = re.compile(r'\s*(\.section\s+\.AMDGPU\.gpr_maximums|\.amdgpu_metadata|\.type\s.*@object)')  # after the last function
index = re.compile(r'(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\.LCPI)\d+')
def functions(path):
    out, cur = {}, None
    if not os.path.exists(path): return out
    for line in open(path):
        m = begin.search(line)
        if m:
            while cur and lead.match(cur[-1]): cur.pop()          # the next function's .section / .protected lines
            cur = out.setdefault(m.group(1), [])
        elif tail.match(line): cur = None
        elif cur is not None: cur.append(' '.join(index.sub(r'\1#', line).split()))   # (comments are padded to a column)
    return out
def pretty(syms):
    names = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True).stdout.split('\n')
    return [re.sub(r'\(anonymous namespace\)::', '', n) for n in names[:len(syms)]]
bad = 0
for name in sorted(set(os.listdir(old_dir)) | set(os.listdir(new_dir))):
    old, new = functions(os.path.join(old_dir, name)), functions(os.path.join(new_dir, name))
    differ = [s for s in old if s in new and old[s] != new[s]]
    gone, added = [s for s in old if s not in new], [s for s in new if s not in old]
    print(f'{name[:-2]}.hip: {len(old)} kernels old, {len(new)} new, {len(differ)} differ, {len(gone)} only old, {len(added)} only new')
    for what, syms in (('differs', differ), ('only in the old tree', gone), ('only in the new tree', added)):
        for n in pretty(syms): print(f'  {what}: {n}')
    bad += len(differ) + len(added)
sys.exit(1 if bad else 0)
" "$tmp/asm_old" "$tmp/asm_new"
