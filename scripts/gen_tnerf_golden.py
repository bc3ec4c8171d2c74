#!/usr/bin/env python3
"""Writes tests/golden/ref_tnerf.npz from the reference's own ``TNeRFRadianceField`` (examples/radiance_fields/mlp.py), on the CPU:
    python scripts/gen_tnerf_golden.py /path/to/the/reference/checkout
Three fields (tests/tnerf_field_reference.py: FIELDS), run in float64 on N = 48 rows (x in +-1, t in [0, 1], unit directions;
float32 numbers, stored): `ref`, the class as it is (trunk 8 x 256, input appended after hidden layer 4); `small`, the same class
with its `nerf` replaced by the reference's VanillaNeRFRadianceField(net_depth=2, net_width=128); `perm`, `small` with the perm
family in the warp network, whose deformation is 0, 1 or 2 times one column of the encoded row, so that the bound on the warped
positions is a rounding of the half type and a wrong warp stage misses it by three orders of magnitude.  The weights are NOT
stored: reference_state_dict there makes them by deterministic rules and the fixture holds their checksum.  Stored per field
`<name>/`: `checksum`, and the reference's `rgb`, `sigma` (forward), `density` (query_density) and `warped` (x + warp(...)) as
float32; once: `x`, `t`, `dir`.  Data only; no test imports this script."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlp_stream_reference as Q  # noqa: E402
import tnerf_field_reference as T  # noqa: E402

N = 48


def inputs():
    gen = torch.Generator().manual_seed(3)
    x, t = torch.rand(N, 3, generator=gen) * 2 - 1, torch.rand(N, 1, generator=gen)
    return x, t, torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)


def main():
    spec = importlib.util.spec_from_file_location("ref_mlp", os.path.join(sys.argv[1], "examples", "radiance_fields", "mlp.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    x, t, d = inputs()
    out = {"x": x.numpy(), "t": t.numpy(), "dir": d.numpy()}
    for name, (depth, width, skip, _) in T.FIELDS.items():
        f = ref.TNeRFRadianceField()
        f.nerf = ref.VanillaNeRFRadianceField(net_depth=depth, net_width=width, skip_layer=skip)
        sd = T.reference_state_dict(name)
        missing, unexpected = f.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith(".scales") for k in missing), (missing, unexpected)
        f = f.double()
        with torch.no_grad():
            rgb, sigma = f(x.double(), t.double(), d.double())
            density = f.query_density(x.double(), t.double())
            warped = (x.double() + f.warp(torch.cat([f.posi_encoder(x.double()), f.time_encoder(t.double())], -1)))
        out[name + "/checksum"] = np.float64(Q.checksum(sd))
        for k, v in (("rgb", rgb), ("sigma", sigma), ("density", density), ("warped", warped)):
            out[f"{name}/{k}"] = v.numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "ref_tnerf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
