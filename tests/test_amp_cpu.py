"""CPU-side checks of the loss-scaling entry points (cer_amp_check_unscale_flat, cer_sgd_nesterov_flat_amp,
cer_adam_flat_amp) and of the optimisers' GradScaler contract.  Every call below is refused by the argument checks before
any launch, so no GPU is needed (and none is touched)."""
import ctypes

import pytest
import torch

A = ctypes.c_void_p(1 << 20)          # 16-byte aligned, never dereferenced: each call fails its checks first
MIS = ctypes.c_void_p((1 << 20) + 4)  # 4-byte aligned only
ODD = ctypes.c_void_p((1 << 20) + 2)


def _lib():
    from feature_vs_text_compound_emotion_amd import _lib
    from feature_vs_text_compound_emotion_amd.build import build
    build(verbose=False)
    return _lib.load()


def _refused(lib, rc, what):
    assert rc == -1
    msg = lib.cer_last_error()
    assert msg and what.encode() in msg, msg


def test_check_unscale_refuses_null_and_misaligned_pointers():
    lib = _lib()
    _refused(lib, lib.cer_amp_check_unscale_flat(None, 8, None, A, None), "amp_check_unscale_flat")     # no grad
    _refused(lib, lib.cer_amp_check_unscale_flat(A, 8, None, None, None), "amp_check_unscale_flat")     # no found_inf
    _refused(lib, lib.cer_amp_check_unscale_flat(A, 6, None, A, None), "amp_check_unscale_flat")        # n % 4
    _refused(lib, lib.cer_amp_check_unscale_flat(A, 0, None, A, None), "amp_check_unscale_flat")        # n == 0
    _refused(lib, lib.cer_amp_check_unscale_flat(MIS, 8, None, A, None), "amp_check_unscale_flat")      # grad not float4
    _refused(lib, lib.cer_amp_check_unscale_flat(A, 8, ODD, A, None), "amp_check_unscale_flat")         # inv_scale
    _refused(lib, lib.cer_amp_check_unscale_flat(A, 8, None, ODD, None), "amp_check_unscale_flat")      # found_inf


def test_sgd_amp_refuses_null_and_misaligned_pointers():
    lib = _lib()
    f = lib.cer_sgd_nesterov_flat_amp
    ok = dict(lr=1e-3, mu=0.9, damp=0.0, wd=1e-4, nesterov=1)

    def call(param=A, grad=A, buf=A, n=8, grad_scale=A, found_inf=A, applied=A, **kw):
        a = dict(ok, **kw)
        return f(param, grad, buf, n, a["lr"], a["mu"], a["damp"], a["wd"], a["nesterov"], grad_scale, found_inf, applied, None)
    for bad in (dict(param=None), dict(grad=None), dict(buf=None), dict(n=6), dict(n=0), dict(found_inf=None),
                dict(applied=None), dict(param=MIS), dict(grad=MIS), dict(buf=MIS), dict(grad_scale=ODD),
                dict(found_inf=ODD), dict(applied=MIS), dict(damp=0.1), dict(mu=0.0)):
        _refused(lib, call(**bad), "sgd_nesterov_flat_amp")


def test_adam_amp_refuses_null_and_misaligned_pointers():
    lib = _lib()
    f = lib.cer_adam_flat_amp

    def call(param=A, grad=A, m=A, v=A, vmax=A, n=8, beta1=0.9, beta2=0.999, amsgrad=1, table=A, table_len=4, grad_scale=A,
             found_inf=A, applied=A):
        return f(param, grad, m, v, vmax, n, 1e-3, beta1, beta2, 1e-8, 0.0, amsgrad, table, table_len, grad_scale, found_inf,
                 applied, None)
    for bad in (dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(vmax=None), dict(n=6), dict(n=0),
                dict(table=None), dict(table_len=0), dict(found_inf=None), dict(applied=None), dict(param=MIS),
                dict(m=MIS), dict(vmax=MIS), dict(table=MIS), dict(grad_scale=ODD), dict(found_inf=ODD), dict(applied=MIS),
                dict(beta1=1.0), dict(beta2=-0.1)):
        _refused(lib, call(**bad), "adam_flat_amp")


def test_wrappers_refuse_cpu_tensors():
    from feature_vs_text_compound_emotion_amd import ops
    with pytest.raises(ValueError):
        ops.amp_check_unscale_flat(torch.zeros(8), torch.zeros(()))
    z = torch.zeros(8)
    with pytest.raises(ValueError):
        ops.sgd_nesterov_flat_amp(z, z, z, 1e-3, None, torch.zeros(()), torch.zeros((), dtype=torch.int64))


def test_flat_optimisers_declare_the_grad_scaler_contract():
    """torch.amp.GradScaler.step hands ``grad_scale`` / ``found_inf`` to an optimiser only if it declares
    ``_step_supports_amp_scaling`` and its ``step`` takes no ``grad_scaler`` argument (the deprecated form)."""
    import inspect
    from feature_vs_text_compound_emotion_amd.data_parallel import FlatAdam, FlatGradScaler, FlatNesterovSGD
    for cls in (FlatNesterovSGD, FlatAdam):
        assert cls._step_supports_amp_scaling is True
        assert "grad_scaler" not in inspect.signature(cls.step).parameters
    assert issubclass(FlatGradScaler, torch.amp.GradScaler)
    # the private hooks FlatGradScaler overrides exist with these signatures in the installed torch
    sig = inspect.signature(torch.amp.GradScaler._unscale_grads_)
    assert list(sig.parameters) == ["self", "optimizer", "inv_scale", "found_inf", "allow_fp16"]
    assert list(inspect.signature(torch.amp.GradScaler._check_inf_per_device).parameters) == ["self", "optimizer"]
    assert hasattr(torch.amp.GradScaler, "_check_scale_growth_tracker")
