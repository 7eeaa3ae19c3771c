"""Generates tests/golden/fountain11_skeleton.bin.xz and fountain11_archive.json from the reference fixture.

    python tests/golden/make_fountain11_skeleton.py <reference checkout>/data/sfm/fountain11.bin

The archive itself is too large to keep here, but most of its bytes are doubles that fountain11_flat.npz already holds
verbatim: the points of the tracks and the image coordinates of their observations.  The skeleton is the archive with
exactly those doubles set to zero; tests/test_io_roundtrip.py fills them back in from the npz and checks that the
result is the reference's file byte for byte (size and SHA-256 recorded here).
"""
import hashlib
import json
import lzma
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from theiasfm_amd import io  # noqa: E402

src = sys.argv[1]
raw = open(src, "rb").read()
rec = io.read_theia_reconstruction(src)
prob = io.flatten_reconstruction(rec)
gold = np.load(os.path.join(HERE, "fountain11_flat.npz"))
assert (prob.points == gold["points"]).all() and (prob.obs_xy == gold["obs_xy"]).all()
vids, tids = prob.meta["view_ids"], prob.meta["track_ids"]
for t in tids:
    rec.tracks[t].point = np.zeros(4)
for c, p in zip(prob.obs_camera, prob.obs_point):
    rec.views[vids[c]].features[tids[p]] = (0.0, 0.0)
skeleton = os.path.join(HERE, "fountain11_skeleton.bin")
io.write_theia_reconstruction(skeleton, rec)
with open(skeleton, "rb") as fh:
    data = fh.read()
os.remove(skeleton)
with open(skeleton + ".xz", "wb") as fh:
    fh.write(lzma.compress(data, preset=9))
json.dump(dict(size=len(raw), sha256=hashlib.sha256(raw).hexdigest(), source="data/sfm/fountain11.bin"),
          open(os.path.join(HERE, "fountain11_archive.json"), "w"), indent=1)
