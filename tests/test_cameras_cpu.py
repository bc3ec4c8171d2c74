"""CPU: nerfacc_amd.cameras -- the reference's five names, the torch models against the reference's outputs
(tests/golden/cameras.npz, scripts/gen_camera_golden.py), and the C ABI's argument checks."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

# ref: nerfacc/cameras.py: (name, default) of every positional-or-keyword parameter
REFERENCE_SIGNATURES = {
    "opencv_lens_undistortion": [("uv", None), ("params", None), ("eps", 1e-6), ("iters", 10)],
    "opencv_lens_undistortion_fisheye": [("uv", None), ("params", None), ("eps", 1e-6), ("iters", 10)],
    "_opencv_lens_distortion": [("uv", None), ("params", None)],
    "_opencv_lens_distortion_fisheye": [("uv", None), ("params", None), ("eps", 1e-10)],
    "_opencv_lens_undistortion": [("uv", None), ("params", None), ("eps", 1e-6), ("iters", 10)],
}


def _cases():
    g = load_golden("cameras")
    return g, [i for i in range(int(g["n_cases"]))]


def test_cameras_module_exposes_reference_names():
    import nerfacc_amd
    from nerfacc_amd import cameras
    for name, sig in REFERENCE_SIGNATURES.items():
        params = inspect.signature(getattr(cameras, name)).parameters.values()
        assert all(q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for q in params), name
        got = [(q.name, None if q.default is inspect.Parameter.empty else q.default) for q in params]
        assert got == sig, (name, got)
        assert name not in nerfacc_amd.__all__   # reached as nerfacc_amd.cameras, as in the reference


def test_torch_models_match_reference_fixture():
    from nerfacc_amd import cameras as cam
    g, cases = _cases()
    eps, iters = float(g["eps"]), int(g["iters"])
    for i in cases:
        uv, p, fe = (torch.from_numpy(g[f"c{i}_{k}"]) for k in ("uv", "params", "fe_params"))
        p8 = F.pad(p, (0, 8 - p.shape[-1]))
        np.testing.assert_allclose(cam._opencv_lens_undistortion(uv, p, eps, iters).numpy(), g[f"c{i}_undist"], atol=1e-6,
                                   rtol=0, err_msg=f"case {i} undistortion")
        np.testing.assert_allclose(cam._opencv_lens_distortion(uv, p8).numpy(), g[f"c{i}_dist"], atol=1e-6, rtol=0,
                                   err_msg=f"case {i} distortion")
        np.testing.assert_allclose(cam._opencv_lens_distortion_fisheye(uv, fe).numpy(), g[f"c{i}_fe_dist"], atol=1e-6,
                                   rtol=0, err_msg=f"case {i} fisheye distortion")


def test_torch_undistortion_round_trips():
    from nerfacc_amd import cameras as cam
    g, cases = _cases()
    for i in cases:
        uv, p = torch.from_numpy(g[f"c{i}_uv"]), torch.from_numpy(g[f"c{i}_params"])
        und = cam._opencv_lens_undistortion(uv, p, float(g["eps"]), int(g["iters"]))
        back = cam._opencv_lens_distortion(und, F.pad(p, (0, 8 - p.shape[-1])))
        assert float((back - uv).abs().max()) <= 1e-5, i


def test_torch_undistortion_without_parameters_is_identity():
    from nerfacc_amd import cameras as cam
    uv = torch.rand(5, 2)
    assert cam._opencv_lens_undistortion(uv, torch.zeros(0)) is uv


@pytest.mark.parametrize("fn", ["nfa_opencv_lens_undistortion", "nfa_opencv_lens_undistortion_fisheye"])
def test_lens_abi_rejects_bad_arguments(fn):
    from nerfacc_amd import _backend as B
    lib = B.load()
    f = getattr(lib, fn)
    good = 4 if fn.endswith("fisheye") else 8
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def err(*args):
        rc = f(*args)
        assert rc == -1, (args, rc)   # NFA_EINVAL
        return lib.nfa_last_error().decode()

    assert "null pointer" in err(None, p, 4, good, 0, 1e-6, 10, p, None)
    assert "null pointer" in err(p, None, 4, good, 0, 1e-6, 10, p, None)
    assert "null pointer" in err(p, p, 4, good, 0, 1e-6, 10, None, None)
    for n_params in (3, 6, 13):
        assert "n_params" in err(p, p, 4, n_params, 0, 1e-6, 10, p, None)
    assert "iters" in err(p, p, 4, good, 0, 1e-6, -1, p, None)
    assert "param_stride" in err(p, p, 4, good, 3, 1e-6, 10, p, None)
    assert "negative" in err(p, p, -1, good, 0, 1e-6, 10, p, None)
    # nothing to do: no launch, no device needed, null pointers allowed
    assert f(None, None, 0, good, 0, 1e-6, 10, None, None) == 0
    assert f(None, None, 0, good, good, 1e-6, 0, None, None) == 0


def test_native_wrappers_refuse_cpu_tensors():
    from nerfacc_amd import cameras as cam
    uv = torch.rand(10, 2)
    with pytest.raises(NotImplementedError):
        cam.opencv_lens_undistortion(uv, torch.rand(8) * 0.01)
    with pytest.raises(NotImplementedError):
        cam.opencv_lens_undistortion(uv, torch.rand(10, 2) * 0.01)
    with pytest.raises(NotImplementedError):
        cam.opencv_lens_undistortion_fisheye(uv, torch.rand(4) * 0.01)
    assert cam.opencv_lens_undistortion(uv, torch.zeros(0)) is uv   # N = 0 returns the input without a device
    with pytest.raises(ValueError):
        cam.opencv_lens_undistortion(uv, torch.rand(3))
    with pytest.raises(ValueError):
        cam.opencv_lens_undistortion_fisheye(uv, torch.rand(5))


def test_compat_lens_functions_check_inputs():
    import nerfacc_amd.cuda_compat as _C
    uv = torch.rand(10, 2)
    with pytest.raises(RuntimeError):
        _C.opencv_lens_undistortion(uv, torch.rand(10, 8), 1e-6, 10)   # CPU tensors (CHECK_INPUT)
    with pytest.raises(RuntimeError):
        _C.opencv_lens_undistortion_fisheye(uv, torch.rand(10, 4), 1e-6, 10)
