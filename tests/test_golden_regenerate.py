"""The pin of the integer IM chain: tests/golden/make_golden.py imports the REAL reference (IMK_REFERENCE=<checkout>, its cv2 /
tensorflow imports stubbed, every exercised function pure numpy), writes the fixtures the parity tests compare against and records a
sha256 of every array of every fixture in tests/golden/digests.json.  This test requires the committed fixtures to be exactly what that
regeneration recorded: every fixture present, no array added, dropped or changed without regenerating from the reference.
SURVEY 8c; functions.py:3104-3238, 2832-2891, 2988-3070, 4328-4459, 1463-1478."""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("im_binary", "im_hela", "im_multiclass", "writer_isic", "writer_multi", "metrics", "augment", "evalnet_labels")


def array_digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str}|{a.shape}|".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def test_fixtures_equal_what_the_reference_regeneration_recorded():
    with open(os.path.join(GOLD, "digests.json")) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(FIXTURES), sorted(rec)
    for name in FIXTURES:
        with np.load(os.path.join(GOLD, name + ".npz")) as d:
            assert sorted(d.files) == sorted(rec[name]), name
            for k in d.files:
                assert array_digest(d[k]) == rec[name][k], (name, k)
