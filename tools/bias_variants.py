#!/usr/bin/env python3
"""
The bias fit's alternatives, built and timed: what DESIGN section 4.35 chose its shape by.

    python tools/bias_variants.py --build            # needs no GPU: tools/_variants/lkamd_bias_*.so
    python tools/bias_variants.py [--out FILE]       # times them, one fresh process each

``csrc/bias.hip`` takes its two seams and the chain's step from macros: ``LK_BIAS_SHORT`` (bins up
to this length are one lane's; 64), ``LK_BIAS_CHUNK`` (what the wave of a longer bin loads at a
time; 256) and ``LK_BIAS_LDS`` (1: the chunk's values are laid in LDS as float64 and the chain
reads them there instead of ``v_readlane`` + convert; 0).  ``--build`` compiles ``bias.hip`` once
per variant and links it with the objects of the ordinary build.  The timing run loads each
library through ``LK_AMD_LIBRARY`` in a child process and, at the ML-25M shape with damping 100/3,
times the item pass, the user pass and the longest item's bin alone (best of seven, matrices in
HBM), and checks the biases against the default build's by bits.  One JSON document.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT_DIR = ROOT / "tools" / "_variants"
VARIANTS = {"default": [], "short32": ["-DLK_BIAS_SHORT=32"], "short128": ["-DLK_BIAS_SHORT=128"],
            "chunk128": ["-DLK_BIAS_CHUNK=128"], "chunk512": ["-DLK_BIAS_CHUNK=512"],
            "lds": ["-DLK_BIAS_LDS=1"]}


def _lib(name: str) -> Path:
    return OUT_DIR / f"lkamd_bias_{name}.so"


def build():
    from lkpy_amd.csrc import build as B

    B.build()
    OUT_DIR.mkdir(parents=True, exist_ok=True)
    rest = [str(o) for o in sorted(B.OBJ.glob("*.o")) if o.name != "bias.o"]
    for name, flags in VARIANTS.items():
        obj = OUT_DIR / f"bias_{name}.o"
        subprocess.check_call([B.HIPCC, *flags, *B.FLAGS, "-c", str(B.HERE / "bias.hip"), "-o",
                               str(obj)])
        subprocess.check_call([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o",
                               str(_lib(name)), *rest, str(obj)])
        print("built", _lib(name))


def child():
    "one library (``LK_AMD_LIBRARY``): a JSON line of times and a digest of the biases"
    import hashlib

    import numpy as np
    import torch

    import bias_time as T
    from lkpy_amd import _device as D
    from lkpy_amd import _native, synth

    m = synth.ml25m_like()
    dev = D.device()
    csr = D.DeviceCSR.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
    csr_t = D.csr_transpose(csr, with_values=True)
    g = float(np.mean(m.data))
    ib, ub = D.bias_fit(csr, csr_t, g, T.DAMPING, T.DAMPING)
    item, _ = T._best(lambda: D.bias_fit(csr, csr_t, g, T.DAMPING, T.DAMPING, users=False), 7)
    user, _ = T._best(lambda: T._user_pass(D, csr, g, ib), 7)
    t_ptr = csr_t.indptr.cpu().numpy()
    top = int(np.diff(t_ptr).argmax())
    s, e = int(t_ptr[top]), int(t_ptr[top + 1])
    one = D.DeviceCSR(torch.tensor([0, e - s], dtype=torch.int64, device=dev),
                      csr_t.indices[s:e].contiguous(), csr_t.values[s:e].contiguous(),
                      (1, m.shape[0]), None)
    lone, _ = T._best(lambda: T._one_bin(D, one, g), 7)
    lib = _native.load()
    digest = hashlib.sha256(ib.cpu().numpy().tobytes() + ub.cpu().numpy().tobytes()).hexdigest()
    print(json.dumps({"short_max": int(lib.lk_bias_fit_short_max()),
                      "chunk": int(lib.lk_bias_fit_chunk()), "item_pass_seconds": item,
                      "user_pass_seconds": user, "longest_item_chain_alone_seconds": lone,
                      "longest_item": e - s, "biases_sha256": digest}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.build:
        return build()
    if args.child:
        return child()
    res = {}
    for name in VARIANTS:
        if not _lib(name).exists():
            raise SystemExit(f"{_lib(name)} is missing: run with --build first")
        env = dict(os.environ, LK_AMD_LIBRARY=str(_lib(name)))
        done = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env,
                              capture_output=True, text=True, timeout=300)
        if done.returncode != 0:  # nothing more is started on the device after a failure
            res[name] = {"failed": done.returncode, "stderr": done.stderr[-2000:]}
            break
        res[name] = json.loads(done.stdout.strip().splitlines()[-1])
        res[name]["same_bits_as_default"] = \
            res[name]["biases_sha256"] == res["default"]["biases_sha256"]
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 1 if any("failed" in v for v in res.values()) else 0


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT / "tools"))
    sys.exit(main() or 0)
