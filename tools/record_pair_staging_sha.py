"""Record the sha256 of the output bytes of the seeded staging cases
(tests/pair_staging_cases.py: SHA_CASES) for the build in the current
directory.

tests/golden/pair_staging_parent_sha256.json holds the values of the commit
BEFORE the batched staging, recorded on an MI355X.  To re-record, check that
commit out somewhere, build it, and run this file (of the current tree) from
the root of that checkout:

    cd <checkout of the parent commit>
    python -c "import __graft_entry__ as g; g.build()"
    python <this tree>/tools/record_pair_staging_sha.py --out <json>

Never run it on the code under test to refresh the golden file: that turns
the test into a comparison of the code with itself.  With --check PATH it
compares instead of writing and exits 1 on a difference.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, '.')  # the build under measurement: the current directory
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', 'tests'))
import pair_staging_cases as pc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--check", default=None)
ap.add_argument("--commit", default="",
                help="commit id of the build, stored in the file")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda:0")
import sonata_amd  # noqa: E402

print(f"# build under {os.path.dirname(os.path.abspath(sonata_amd.__file__))}")
sha = {}
for name in sorted(pc.SHA_CASES):
    a = pc.SHA_CASES[name](dev)
    b = pc.SHA_CASES[name](dev)
    torch.cuda.synchronize()
    assert pc.sha256_of(a) == pc.sha256_of(b), f"{name}: two runs differ"
    sha[name] = pc.sha256_of(a)
    print(f"{name}: {sha[name]}", flush=True)
if args.check:
    with open(args.check) as f:
        want = json.load(f)["sha256"]
    bad = sorted(n for n in sha if want.get(n) != sha[n])
    print("differing:", bad if bad else "none")
    sys.exit(1 if bad or set(want) != set(sha) else 0)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit,
                   "device": torch.cuda.get_device_name(0),
                   "sha256": sha}, f, indent=1, sort_keys=True)
        f.write("\n")
