"""CPU: the checker of the one-launch eval-mode generators (tests/mmgan_gen_eval_ref.py) accepts a torch emulation of
the kernel's arithmetic and rejects every planted fault, at every geometry of the GPU table; the host-side argument
checks of the C ABI (no launch is made)."""
import ctypes

import pytest
import torch

import mmgan_gen_eval_ref as G
import mmgan_ref as R

B = 2 * G.ROW_TILE + 1


def _case(name, broadcast=False):
    z, n_in, _n4 = G.GEOMETRIES[name]
    return G.make_inputs(B, z, n_in, 7, broadcast=broadcast), G.make_params(name)


@pytest.mark.parametrize("name", G.GEOMETRIES)
def test_parameters_are_calibrated(name):
    """the outputs span more than 0.2 ... 0.8 and running_var is not 1: a constant 0.5 or an identity BatchNorm fails"""
    (noise, inp), params = _case(name)
    out = G.chain_ref(noise, inp, params)[3][2]
    assert float(out.min()) < 0.2 and float(out.max()) > 0.8, (float(out.min()), float(out.max()))
    for p in params:
        assert float((p["running_var"] - 1).abs().min()) > 1e-4
    half = dict(ys=[c[0].float() for c in G.chain_ref(noise, inp, params)],
                acts=[c[2].float() for c in G.chain_ref(noise, inp, params)[:3]], out=torch.full_like(out, 0.5).float())
    with pytest.raises(R.CheckError):
        G.check_run(half, noise, inp, params)


@pytest.mark.parametrize("name", G.GEOMETRIES)
def test_out_bound_is_linear_bn_refs_on_an_exact_input(name):
    (noise, inp), params = _case(name)
    x = G.cat_input(noise, inp).double()
    for p in params:
        lr = G.layer_ref(x, p)
        Ey = G.y_bound(x, torch.zeros_like(x), p)
        torch.testing.assert_close(Ey, lr["y"][1], rtol=1e-12, atol=0)
        torch.testing.assert_close(G.out_bound(lr["y"][0], lr["y"][1], p), lr["out"][1], rtol=1e-12, atol=0)
        x = lr["out"][0]


@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("name", G.GEOMETRIES)
def test_checker_accepts_the_emulation(name, broadcast):
    (noise, inp), params = _case(name, broadcast)
    worst = G.check_run(G.emulate(noise, inp, params), noise, inp, params, what=name)
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("fault", G.FAULTS)
@pytest.mark.parametrize("name", G.GEOMETRIES)
def test_checker_rejects_every_planted_fault(name, fault):
    (noise, inp), params = _case(name, broadcast=fault == "broadcast_noise")
    with pytest.raises(R.CheckError):
        G.check_run(G.emulate(noise, inp, params, faults=(fault,)), noise, inp, params, what=f"{name} {fault}")


def test_the_float64_chain_passes_itself_rounded_to_fp32():
    (noise, inp), params = _case("g2_checkpoint")
    chain = G.chain_ref(noise, inp, params)
    got = dict(ys=[c[0].float() for c in chain], acts=[c[2].float() for c in chain[:3]], out=chain[3][2].float())
    G.check_run(got, noise, inp, params, chain=chain)


# ------------------------------------------------------------------------------------------- host-side argument checks
def test_supported_range_and_pack_bytes():
    from gan_des_midi_music_gen_amd import _lib
    lib = _lib.load()
    for z, n_in, n4 in G.GEOMETRIES.values():
        assert lib.gdm_mmgan_gen_eval_supported(z + n_in, 256, 128, 64, n4) == 1
        assert lib.gdm_mmgan_gen_eval_pack_bytes(z + n_in, 256, 128, 64, n4) % 16 == 0
    assert lib.gdm_mmgan_gen_eval_supported(1, 256, 128, 64, 1) == 1
    assert lib.gdm_mmgan_gen_eval_supported(512, 256, 128, 64, 4096) == 1
    for bad in ((513, 256, 128, 64, 16), (0, 256, 128, 64, 16), (100, 128, 64, 32, 16), (100, 256, 128, 64, 0)):
        assert lib.gdm_mmgan_gen_eval_supported(*bad) == 0
        assert lib.gdm_mmgan_gen_eval_pack_bytes(*bad) == 0
    # K1 = 100 -> 128, N4 = 20 -> 32: hi and lo bf16 images plus five fp32 vectors per layer
    want = sum(kp * np_ * 4 + np_ * 20 for kp, np_ in ((128, 256), (256, 128), (128, 64), (64, 32)))
    assert lib.gdm_mmgan_gen_eval_pack_bytes(100, 256, 128, 64, 20) == want


def test_entry_points_validate_on_the_host_before_any_launch():
    from gan_des_midi_music_gen_amd import _lib
    lib = _lib.load()
    rc = lib.gdm_mmgan_gen_eval_pack(None, None, None, None, None, None, 513, 256, 128, 64, 16, 1e-5, None, 0, None)
    assert rc == -1 and b"not supported" in lib.gdm_last_error()
    rc = lib.gdm_mmgan_gen_eval_pack(None, None, None, None, None, None, 100, 256, 128, 64, 16, 1e-5, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.gdm_last_error()
    assert lib.gdm_mmgan_gen_eval(None, 1, 256, 128, 64, None) == -1
    jobs = (_lib.MmganGenEvalJob * 2)()
    as_p = ctypes.cast(jobs, ctypes.c_void_p)
    assert lib.gdm_mmgan_gen_eval(as_p, 3, 256, 128, 64, None) == -1 and b"1 or 2 jobs" in lib.gdm_last_error()
    j = jobs[0]
    j.B, j.z, j.in_, j.n4, j.input_stride = 0, 50, 50, 20, 50
    assert lib.gdm_mmgan_gen_eval(as_p, 1, 256, 128, 64, None) == -1 and b"batch" in lib.gdm_last_error()
    j.B = 4
    assert lib.gdm_mmgan_gen_eval(as_p, 1, 128, 64, 32, None) == -1 and b"not supported" in lib.gdm_last_error()
    j.z = 500
    assert lib.gdm_mmgan_gen_eval(as_p, 1, 256, 128, 64, None) == -1 and b"not supported" in lib.gdm_last_error()
    j.z = 50
    assert lib.gdm_mmgan_gen_eval(as_p, 1, 256, 128, 64, None) == -1 and b"null pointer" in lib.gdm_last_error()
    # non-null pointers are never dereferenced on the host: the remaining checks are reached with dummies
    dummy = 4096
    j.noise = j.input = j.pack = j.out = dummy
    j.input_stride = 7
    assert lib.gdm_mmgan_gen_eval(as_p, 1, 256, 128, 64, None) == -1 and b"input_stride" in lib.gdm_last_error()
    j.input_stride = 0
    j.pack_bytes = 16
    assert lib.gdm_mmgan_gen_eval(as_p, 1, 256, 128, 64, None) == -1 and b"pack of 16 bytes" in lib.gdm_last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    from gan_des_midi_music_gen_amd import ops
    layers = [tuple(p[k] for k in ("w",) + G.VEC_NAMES) for p in G.make_params("edge")]
    with pytest.raises(ops.GdmError):
        ops.mmgan_gen_eval_pack(layers)
    with pytest.raises(ops.GdmError):
        ops.mmgan_gen_eval([dict(noise=torch.zeros(2, 3), input=torch.zeros(2, 4), pack=torch.zeros(16, dtype=torch.uint8),
                                 dims=(7, 256, 128, 64, 17))])
