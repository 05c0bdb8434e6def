#!/bin/bash
# Build libdawn_hip.so for gfx950 (cross-compiles without a GPU; incremental).  In-tree output so it ships with the tree.
# The recipe (sources, flags, instrumented variants) lives in hipbuild.py.
exec python3 "$(dirname "$0")/hipbuild.py" "$@"
