#!/bin/bash
# Same device code as a git revision?  Compiles each HIP source of csrc/ as it is at <rev> (with
# that revision's headers) and as it is in the working tree, device-only to gfx950 assembly, and
# diffs the instruction text (comments, directives and the per-build __hip_cuid_ symbol removed).
# usage: bash tools/isa_same.sh [--per-kernel] <rev> [file.hip ...]     (default: the .hip files
# that differ from <rev>, or all of them when a header differs)
# env: JOBS = parallel compiles (default 4)
# Prints "identical" / "NOT identical" per file; the assembly and the diffs stay in $OUT
# (default /tmp/isa_same).  Exit status 1 if any file differs.
# --per-kernel: for a change that removes kernels.  Each file's instruction text is split at its
# function symbols and the functions are compared by name, with the local labels (.LBB<n>_<m>,
# .Ltmp<k>, .Lfunc_end<n>: numbered per file, so they shift when other kernels go) renumbered per
# function.  Passes when every function of the working tree exists at <rev> with the same text;
# functions only at <rev> are listed as removed and do not fail the check.
set -o pipefail
per_kernel=0
if [ "$1" = "--per-kernel" ]; then per_kernel=1; shift; fi
rev=${1:?usage: isa_same.sh [--per-kernel] <rev> [file.hip ...]}; shift
root=$(git rev-parse --show-toplevel) || exit 2
src=deep_video_interpolation_extrapolation_amd/csrc
out=${OUT:-/tmp/isa_same}; jobs=${JOBS:-4}
cd "$root" || exit 2
files=("$@")
if [ ${#files[@]} -eq 0 ]; then
  if git diff --name-only "$rev" -- $src include | grep -q '\.h$' || [ -n "$(git ls-files -o --exclude-standard $src | grep '\.h$')" ]; then
    files=($(cd $src && ls *.hip))
  else
    files=($(git diff --name-only "$rev" -- $src | grep '\.hip$' | xargs -r -n1 basename))
  fi
fi
rm -rf "$out"; mkdir -p "$out/old" "$out/new"
git archive "$rev" $src include | tar -x -C "$out/old" || exit 2
flags="--offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -S"
for f in "${files[@]}"; do
  echo "/opt/rocm/bin/hipcc $flags $out/old/$src/$f -o $out/old/${f%.hip}.s"
  echo "/opt/rocm/bin/hipcc $flags $src/$f -o $out/new/${f%.hip}.s"
done | xargs -P "$jobs" -I{} sh -c "{} 2>>$out/compile.log" || { cat "$out/compile.log"; exit 2; }
# instruction text only: labels and instructions, no comments, no directives, no metadata
strip() {
  sed -e '/^[ \t]*\.amdgpu_metadata/,/^[ \t]*\.end_amdgpu_metadata/d' -e 's/[ \t]*;.*$//' "$1" |
    grep -v -e '^[ \t]*$' -e '__hip_cuid_' | grep -v -E '^[ \t]*\.[A-Za-z_0-9]+([ \t]|$)'
}
# functions of a stripped file, by name: prints "same <n>", "removed <name>", "added <name>",
# "differs <name>" lines; exit status 1 on an added or differing function
by_kernel() {
  python3 - "$1" "$2" <<'PY'
import re, sys
def funcs(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and not re.match(r"^\s*\.(?!L\w+:)", line):  # (no directives: they name the next function)
            out[name].append(line.strip())
    for body in out.values():  # local labels in order of first appearance
        ids = {}
        body[:] = [re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), l)
                   for l in body]
    return out
old, new = funcs(sys.argv[1]), funcs(sys.argv[2])
bad = 0
print("same", sum(1 for k in new if old.get(k) == new[k]))
for k in sorted(old):
    if k not in new: print("removed", k)
for k in sorted(new):
    if k not in old: print("added", k); bad = 1
    elif old[k] != new[k]: print("differs", k); bad = 1
sys.exit(bad)
PY
}
rc=0
for f in "${files[@]}"; do
  b=${f%.hip}
  strip "$out/old/$b.s" > "$out/old/$b.txt"; strip "$out/new/$b.s" > "$out/new/$b.txt"
  if [ $per_kernel = 1 ]; then
    if by_kernel "$out/old/$b.txt" "$out/new/$b.txt" > "$out/$b.kernels"; then
      echo "$f: $(sed -n 's/^same //p' "$out/$b.kernels") functions identical, $(grep -c '^removed' "$out/$b.kernels") only at $rev"
    else
      echo "$f: NOT identical ($out/$b.kernels)"; grep -E '^(added|differs)' "$out/$b.kernels" | c++filt | sed 's/^/  /'; rc=1
    fi
    grep '^removed' "$out/$b.kernels" | c++filt | sed 's/^/  /'
  elif diff "$out/old/$b.txt" "$out/new/$b.txt" > "$out/$b.diff"; then
    echo "$f: identical ($(wc -l < "$out/new/$b.txt") lines)"
  else
    echo "$f: NOT identical ($(grep -c '^[<>]' "$out/$b.diff") differing lines, $out/$b.diff)"; rc=1
  fi
done
exit $rc
