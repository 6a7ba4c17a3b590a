#!/bin/bash
# Diagnostic: build a variant of the product library into build_ab/<name>.so with extra compiler flags, for tools/ab.py.
# The flags and the source list are build.py's.  CHECKOUT=<dir>: the sources of another checkout of the repository (a
# `git worktree` of the commit to compare with) instead of this one's.
# usage: [CHECKOUT=<dir>] tools/build_variant.sh <name> [flags ...]
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build_ab
python -m corintho_ai_amd.build --out "build_ab/$name.so" "${CHECKOUT:-.}/corintho_ai_amd/csrc" "$@" | tail -n 1
