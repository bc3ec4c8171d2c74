#!/usr/bin/env python3
"""Writes tests/golden/ref_ndr_field.npz from the reference's own ``NDRTNeRFRadianceField`` (examples/radiance_fields/mlp.py), on the
CPU:
    python scripts/gen_ndr_golden.py /path/to/the/reference/checkout
Two fields (tests/ndr_field_reference.py: FIELDS), run in float64 on N = 48 rows (x in +-1, t in [0, 1]; float32 numbers, stored),
both with the class's `nerf` replaced by the reference's VanillaNeRFRadianceField(net_depth=2, net_width=128): `perm`, the perm
family, whose warp is exact in the half types, and `rot`, the same one-term matrices with a non-zero rotation angle and a bias on
every layer.  For both the bound on the warped positions is a few roundings, so a wrong block order, axis roll, rotation sign or
a dropped bias misses it by orders of magnitude.  The weights are NOT stored: reference_state_dict there makes them by
deterministic rules and the fixture holds their checksum.  Stored per field `<name>/`: `checksum` and the reference's `warped`
(warp) as float32; once: `x`, `t`.  Data only; no test imports this script."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlp_stream_reference as Q  # noqa: E402
import ndr_field_reference as R  # noqa: E402

N = 48


def inputs():
    gen = torch.Generator().manual_seed(3)
    return torch.rand(N, 3, generator=gen) * 2 - 1, torch.rand(N, 1, generator=gen)


def main():
    spec = importlib.util.spec_from_file_location("ref_mlp", os.path.join(sys.argv[1], "examples", "radiance_fields", "mlp.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    x, t = inputs()
    out = {"x": x.numpy(), "t": t.numpy()}
    for name, (depth, width, skip, _) in R.FIELDS.items():
        f = ref.NDRTNeRFRadianceField()
        f.nerf = ref.VanillaNeRFRadianceField(net_depth=depth, net_width=width, skip_layer=skip)
        sd = R.reference_state_dict(name)
        missing, unexpected = f.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith(".scales") for k in missing), (missing, unexpected)
        f = f.double()
        with torch.no_grad():
            out[name + "/warped"] = f.warp(x.double(), t.double()).numpy().astype(np.float32)
        out[name + "/checksum"] = np.float64(Q.checksum(sd))
    path = os.path.join(ROOT, "tests", "golden", "ref_ndr_field.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
