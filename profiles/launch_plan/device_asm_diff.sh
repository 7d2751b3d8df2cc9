#!/bin/bash
# The proof that a host-side change left the gfx950 device code alone:
#   profiles/launch_plan/device_asm_diff.sh PARENT_REV [WORKDIR]
# compiles every .hip translation unit that includes an edited header (salamander.hip,
# salamander_inst.hip for the 16 salt words, gecko.hip, udpmsg.hip, addr.hip) with the
# Makefile's flags plus -save-temps=obj, once from PARENT_REV (git archive) and once from
# the working tree, both under WORKDIR, and diffs the gfx950 device assembly files.  Lines
# that carry a path or the compiler's identification (.file, .ident, the bundle's
# comments naming the input) are left out.  Prints one line per file and the number of
# files that differ; exit status 1 when any does.
set -euo pipefail
REV=$1
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
WORK=${2:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result"
JOBS=${JOBS:-8}

mkdir -p "$WORK/parent" "$WORK/new"
[ -d "$WORK/parent/hysteria_amd" ] || git -C "$ROOT" archive "$REV" hysteria_amd/csrc include | tar -x -C "$WORK/parent"
rm -rf "$WORK/new/hysteria_amd" "$WORK/new/include"
mkdir -p "$WORK/new/hysteria_amd/csrc"
cp -r "$ROOT/include" "$WORK/new/"
find "$ROOT/hysteria_amd/csrc" -maxdepth 1 -type f -exec cp {} "$WORK/new/hysteria_amd/csrc/" \;

compile() {   # side
    cd "$WORK/$1/hysteria_amd/csrc"
    [ -d asm ] && return 0
    mkdir -p asm.tmp
    {
        for tu in salamander gecko udpmsg addr; do echo "$HIPCC $FLAGS -c $tu.hip -save-temps=obj -o asm.tmp/$tu.o"; done
        for n in $(seq 0 15); do   # the temporaries are named after the source file: a directory per salt word
            mkdir -p asm.tmp/sw$n
            echo "$HIPCC $FLAGS -DHY_SW=$n -c salamander_inst.hip -save-temps=obj -o asm.tmp/sw$n/salamander_inst.o"
        done
    } | xargs -P "$JOBS" -I{} sh -c '{} 2>>asm.tmp/compile.log'
    mv asm.tmp asm
}
compile parent
compile new

differ=0
total=0
cd "$WORK/parent/hysteria_amd/csrc/asm"
for b in $(find . -name '*gfx950*.s' | sort); do
    b=${b#./}
    f=$WORK/parent/hysteria_amd/csrc/asm/$b
    total=$((total + 1))
    if diff <(grep -vE '^\s*\.(file|ident)\b|^\s*;.*(/|clang version)' "$f") \
            <(grep -vE '^\s*\.(file|ident)\b|^\s*;.*(/|clang version)' "$WORK/new/hysteria_amd/csrc/asm/$b") > "$WORK/${b//\//_}.diff"; then
        echo "identical  $b  ($(wc -l < "$f") lines)"
    else
        echo "DIFFERS    $b  ($(wc -l < "$WORK/${b//\//_}.diff") diff lines, $WORK/${b//\//_}.diff)"
        differ=$((differ + 1))
    fi
done
echo "$total device assembly files compared against $REV, $differ differ"
[ "$differ" -eq 0 ]
