#!/usr/bin/env python3
"""Generate tests/golden/hdf5_h5py.npz: the libhdf5 side of tests/test_hdf5.py, recorded once so that the test
needs no HDF5 installation.

An interpreter that has h5py (libhdf5) is given on the command line.  For the groups of
tests/test_hdf5.py::_groups(n_extra=1500) this script
  1. writes them with this package's writer and checks, through h5py, that libhdf5 reads every dataset back with
     its dtype, shape and values (and, when `h5dump` is given, that it reports the bool masks as the enum over
     H5T_STD_I8LE that h5py writes);
  2. lets h5py write the same groups (what the reference's converter does).
The fixture holds the sha256 of the file of step 1 (`ours_sha256`: the writer must still produce that file byte for
byte) and the bytes of the file of step 2 (`h5py_file`: the reader must read it).

    python tests/golden/make_hdf5_golden.py --h5py-python /path/to/python-with-h5py [--h5dump /path/to/h5dump]
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vqae_amd  # noqa: E402,F401
from vqae_amd import hdf5  # noqa: E402
from test_hdf5 import N_EXTRA_LIBHDF5, _groups  # noqa: E402

CHECK = """
import h5py, numpy as np, sys, warnings
warnings.simplefilter('ignore')
want, ours, theirs = sys.argv[1:4]
z = np.load(want)
with h5py.File(ours, 'r') as f:                          # libhdf5 parses our file
    assert sorted(f.keys()) == ['images', 'masks']
    for k in z.files:
        a = np.asarray(f[k.split('/')[0]][k.split('/')[1]])
        assert a.dtype == z[k].dtype and a.shape == z[k].shape and np.array_equal(a, z[k]), k
    assert sum(len(f[g]) for g in f) == len(z.files)
with h5py.File(theirs, 'w') as f:                        # what the reference's converter does
    for k in z.files:
        g, n = k.split('/')
        f.require_group(g).create_dataset(n, data=z[k])
print('OK')
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h5py-python", required=True, help="an interpreter that can `import h5py`")
    ap.add_argument("--h5dump", default=None, help="libhdf5's h5dump (optional extra check)")
    a = ap.parse_args()
    groups = _groups(n_extra=N_EXTRA_LIBHDF5)
    with tempfile.TemporaryDirectory() as d:
        ours = hdf5.write_hdf5(os.path.join(d, "ours.hdf5"), groups)
        theirs, want = os.path.join(d, "theirs.hdf5"), os.path.join(d, "want.npz")
        np.savez(want, **{f"{g}/{n}": arr for g, ds in groups.items() for n, arr in ds.items()})
        r = subprocess.run([a.h5py_python, "-c", CHECK, want, ours, theirs], capture_output=True, text=True, cwd=d,
                           env={"PATH": "/usr/bin:/bin"})
        if r.returncode != 0 or "OK" not in r.stdout:
            raise SystemExit(f"libhdf5 rejected the writer's file:\n{r.stderr[-2000:]}")
        if a.h5dump:
            r = subprocess.run([a.h5dump, "-H", "-d", "/masks/slide_a_mask", ours], capture_output=True, text=True)
            if r.returncode != 0 or '"TRUE"' not in r.stdout or "H5T_STD_I8LE" not in r.stdout:
                raise SystemExit(f"h5dump: unexpected header of /masks/slide_a_mask:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        ours_sha = hashlib.sha256(open(ours, "rb").read()).hexdigest()
        theirs_bytes = np.frombuffer(open(theirs, "rb").read(), np.uint8)
    path = os.path.join(HERE, "hdf5_h5py.npz")
    np.savez_compressed(path, ours_sha256=np.array(ours_sha), h5py_file=theirs_bytes)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB): writer file sha256 {ours_sha[:16]}..., "
          f"h5py file {theirs_bytes.size} bytes")


if __name__ == "__main__":
    main()
