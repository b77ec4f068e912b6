#!/usr/bin/env python3
"""Writes tests/golden/reference_csharp_surface.json: the public surface (constructors, methods, properties, serialized
fields, Unity messages — names and types only, no code) of the five reference classes SURVEY 8(b) names as the drop-in
boundary, scanned from /root/reference/Assets/_Scripts.  Run in the build container (the reference tree is not on the GPU
box); tests/test_csharp_surface.py compares bindings/csharp/*.Native.cs against this fixture."""
# --check: nothing is written; the committed fixture is compared with a fresh scan (exit status 1 on a difference)
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from csharp_surface import surface          # noqa: E402

REF = "/root/reference/Assets/_Scripts"
FILES = ["DataBuffer.cs", "MeshBufferContainer.cs", "ComputeBufferSorter.cs", "BVHConstructor.cs", "RaytracingMeshDrawer.cs"]

if __name__ == "__main__":
    out = {}
    for f in FILES:
        out[f] = surface(os.path.join(REF, f))
    fixture = os.path.join(HERE, "reference_csharp_surface.json")
    if "--check" in sys.argv[1:]:
        committed = json.load(open(fixture))
        differing = sorted(f for f in set(out) | set(committed) if out.get(f) != committed.get(f))
        print("fixture matches a fresh scan" if not differing else f"fixture differs from a fresh scan in {differing}")
        sys.exit(1 if differing else 0)
    with open(fixture, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
