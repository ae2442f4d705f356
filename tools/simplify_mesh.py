#!/usr/bin/env python
"""Simplify a triangle mesh on the device (multiply_amd/simplify.py: quadric vertex clustering).
    python tools/simplify_mesh.py IN.ply OUT.ply (--cell H | --faces N)
    python tools/simplify_mesh.py IN_DIR OUT_DIR (--cell H | --faces N)
--cell is the cluster size in the mesh's unit; --faces bisects it until the face count (before de-duplication) is within 2 % of N.
With folders every .ply of IN_DIR is written under the same name to OUT_DIR.  Prints one JSON line: counts, cell and bytes before
and after (with folders: {"files": {name: ...}, "total": {...}})."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def jobs_of(src, dst):
    """[(input path, output path)]: the one pair, or for a folder its .ply files by name, sorted"""
    if not os.path.isdir(src):
        return [(src, dst)]
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(".ply") and os.path.isfile(os.path.join(src, f)))
    return [(os.path.join(src, f), os.path.join(dst, f)) for f in names]


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--cell", type=float, default=None, help="cluster size, in the mesh's unit")
    how.add_argument("--faces", type=int, default=None, help="wanted number of faces")
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    jobs = jobs_of(args.src, args.dst)
    if not jobs:
        ap.error("the folder holds no .ply file")
    from multiply_amd import hip, metrics
    from multiply_amd.mesh import ExtractedMesh
    from multiply_amd.simplify import simplify_mesh
    hip.require_device()
    if os.path.isdir(args.src):
        os.makedirs(args.dst, exist_ok=True)
    files = {}
    for src, dst in jobs:
        v, f = metrics.load_ply(src)
        v2, f2, info = simplify_mesh(v, f, cell=args.cell, target_faces=args.faces)
        ExtractedMesh(v2, f2).export(dst)
        files[os.path.basename(src)] = dict(verts_before=int(v.shape[0]), faces_before=int(f.shape[0]), verts_after=int(v2.shape[0]),
                                            faces_after=int(f2.shape[0]), cell=info["cell"], passes=info["passes"],
                                            n_cells=info["n_cells"], n_collapsed=info["n_collapsed"], n_duplicate=info["n_duplicate"],
                                            n_unreferenced=info["n_unreferenced"], bytes_before=os.path.getsize(src),
                                            bytes_after=os.path.getsize(dst))
    if not os.path.isdir(args.src):
        out = files[os.path.basename(args.src)]
    else:
        keys = ("verts_before", "faces_before", "verts_after", "faces_after", "bytes_before", "bytes_after")
        out = dict(files=files, total={k: sum(r[k] for r in files.values()) for k in keys})
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
