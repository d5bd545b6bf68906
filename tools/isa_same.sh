#!/bin/bash
# Same device code as a git revision?  Compiles each HIP source of csrc/ as it is at <rev> (with
# that revision's headers) and as it is in the working tree, device-only to gfx950 assembly, and
# diffs the instruction text (comments, directives and the per-build __hip_cuid_ symbol removed).
# usage: bash tools/isa_same.sh <rev> [file.hip ...]     (default: the .hip files that differ from
# <rev>, or all of them when a header differs)       env: JOBS = parallel compiles (default 4)
# Prints "identical" / "NOT identical" per file; the assembly and the diffs stay in $OUT
# (default /tmp/isa_same).  Exit status 1 if any file differs.
set -o pipefail
rev=${1:?usage: isa_same.sh <rev> [file.hip ...]}; shift
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
rc=0
for f in "${files[@]}"; do
  b=${f%.hip}
  strip "$out/old/$b.s" > "$out/old/$b.txt"; strip "$out/new/$b.s" > "$out/new/$b.txt"
  if diff "$out/old/$b.txt" "$out/new/$b.txt" > "$out/$b.diff"; then
    echo "$f: identical ($(wc -l < "$out/new/$b.txt") lines)"
  else
    echo "$f: NOT identical ($(grep -c '^[<>]' "$out/$b.diff") differing lines, $out/$b.diff)"; rc=1
  fi
done
exit $rc
