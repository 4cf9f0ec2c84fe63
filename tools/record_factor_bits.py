"""Record tests/golden/als_factor_bits.json: the hashes that
tests/test_gpu_als_factor_bits.py compares against, from that file's own input builders.  Run
it on the commit whose bits are to be kept (python tools/record_factor_bits.py [output.json]);
a change that must not move a bit is then tested against the file."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

import test_gpu_als_factor_bits as T  # noqa: E402

for name in T.ENV:
    os.environ.pop(name, None)
dev = torch.device("cuda:0")
out = {}
for case in sorted(T.CASES):
    out[case] = T.CASES[case](dev)
    print(case, out[case], flush=True)
os.environ["LK_ALS_WB_MIN_ROWS"] = "1"
out["k128/woodbury64"] = T.k128_hashes(dev)
print("k128/woodbury64", out["k128/woodbury64"], flush=True)
del os.environ["LK_ALS_WB_MIN_ROWS"]
path = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
path.parent.mkdir(parents=True, exist_ok=True)
path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
print("wrote", path)
