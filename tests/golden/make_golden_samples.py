"""Writes tests/golden/sample_pair/: the DATA of the one real RGB-D pair the reference ships, BASELINE.json configs[0].

    python tests/golden/make_golden_samples.py REFERENCE_TREE

Reads samples/sphere_images_{1,10}.bin (Frame360::serialize's Boost binary archive, Frame360.h:231-266 + cvmat_serialization.h:23-55)
and Calibration/Extrinsics/Rt_0[1-8].txt (Calib360.h:122-131) of the reference tree given on the command line and stores what they hold:

  frame{1,10}_sensors{0-3,4-7}.npz   rgb [4, 240, 320, 3] uint8, depth [4, 240, 320] uint16 (millimetres, 0 = no measurement):
                                     four sensors of one frame per file, so that every file stays under 1 MiB
  Rt_0[1-8].txt                      the sensor -> rig transforms, the reference's text files as they are
  files.json                         size and sha256 of both archives (the 15 version bytes of the Boost header left out) and of the
                                     extrinsics files, so that tests/test_config1_samples.py can prove the fixture equal to them

Inputs only: sensor images and calibration numbers, no source text.  The expected outputs (CRCs of the stitched panoramas, the
oracle's poses and iteration counts, the plane chain's verdict) are tests/golden/config1_samples.json, written by
tests/tools/config1_samples.py --write.  -m gpu tests (tests/test_samples_gpu.py) put this pair through the HIP path.
"""
import hashlib
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def main(ref):
    import config1_samples as c1          # the test-side parser of the archive layout
    out_dir = os.path.join(HERE, "sample_pair")
    os.makedirs(out_dir, exist_ok=True)
    digests = {}
    for idx in (1, 10):
        path = os.path.join(ref, "samples", "sphere_images_%d.bin" % idx)
        frames = c1.load_frame(path)
        for lo in (0, 4):
            np.savez_compressed(os.path.join(out_dir, c1.fixture_part(idx, lo)),
                                rgb=np.stack([f[0] for f in frames[lo:lo + 4]]), depth=np.stack([f[1] for f in frames[lo:lo + 4]]))
        raw = open(path, "rb").read()
        digests["sphere_images_%d.bin" % idx] = {"size": len(raw), "sha256_without_version_bytes": c1.archive_digest(raw)}
    for s in range(8):
        name = "Rt_0%d.txt" % (s + 1)
        shutil.copyfile(os.path.join(ref, "Calibration", "Extrinsics", name), os.path.join(out_dir, name))
        digests[name] = {"sha256": hashlib.sha256(open(os.path.join(out_dir, name), "rb").read()).hexdigest()}
    json.dump(digests, open(os.path.join(out_dir, "files.json"), "w"), indent=1)
    print(out_dir, {f: os.path.getsize(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
