#!/usr/bin/env python
"""Writes tests/golden/helitron_lcvs.json.gz: HelitronScanner's two pattern lists (data files of HiTE that the tool reads at run
time: <HiTE>/bin/HelitronScanner/TrainingSet/head.lcvs and tail.lcvs) as {"head": [lines], "tail": [lines]}, lines in file order,
blank lines dropped, repeated lines kept.  Regenerable byte for byte:
    python tools/gen_helitron_fixture.py [--reference /root/reference]"""
import argparse
import gzip
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HITE_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    src = os.path.join(a.reference, "bin", "HelitronScanner", "TrainingSet")
    obj = {}
    for side in ("head", "tail"):
        with open(os.path.join(src, side + ".lcvs")) as f:
            obj[side] = [ln.strip() for ln in f if ln.strip()]
    path = os.path.join(ROOT, "tests", "golden", "helitron_lcvs.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(obj, separators=(",", ":"), sort_keys=True).encode())
    print("wrote %s: %d head + %d tail lines, %d bytes" % (path, len(obj["head"]), len(obj["tail"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
