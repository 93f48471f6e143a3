"""Host side of the pixel-gradient launchers (no GPU): the C ABI's validation of mia_pgd_update,
mia_grad_assemble and mia_image_grad, and the shape checks of their ops wrappers.

Every C call below is refused before any launch. The checks run in the order null pointers, lo / hi,
S, N, pf, cpad, enc_res, dtype, and a call whose invalid argument an older library would have
launched with (cpad < 3, N or S out of range, lo > hi) also carries an unsupported dtype, the
last check: such a library refuses the call as well, with another message, instead of running a
kernel on the placeholder pointers."""
import ctypes

import pytest
import torch

P = ctypes.c_void_p
BAD_DTYPE = 7


def _abi():
    from gfa_amd import _lib
    lib = _lib.load()
    ok = P(4096)  # never dereferenced: every call below fails validation first

    def expect_einval(name, fragment, *args):
        rc = getattr(lib, name)(*args)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (name, rc, msg)  # MIA_EINVAL
        assert msg.startswith(name + ": ") and fragment in msg, (fragment, msg)
    return expect_einval, ok, P(None)


def _callers():
    """name → call(**overrides) → the entry point with valid defaults (2 images of 32², pf 1,
    8 channels, a 16² encoder gradient, fp32) except the overrides."""
    bad, ok, null = _abi()

    def pgd_update(frag, x=ok, x0=ok, gv=ok, ge=ok, N=2, S=32, pf=1, cpad=8, enc=16, lo=-1.0,
                   hi=1.0, dtype=0):
        bad("mia_pgd_update", frag, x, x0, gv, ge, N, S, pf, cpad, enc, 0.37, 0.03, 0.06, lo, hi,
            null, dtype, null)

    def grad_assemble(frag, x=ok, x0=ok, gv=ok, ge=ok, g=ok, N=2, S=32, pf=1, cpad=8, enc=16,
                      dtype=0):
        bad("mia_grad_assemble", frag, x, x0, gv, ge, g, N, S, pf, cpad, enc, 0.37, 1.0, null,
            dtype, null)

    def image_grad(frag, rec=ok, t=ok, gv=ok, g=ok, N=2, S=32, pf=1, cpad=8, dtype=0):
        bad("mia_image_grad", frag, rec, t, gv, g, N, S, pf, cpad, 0.37, dtype, null)
    return dict(pgd_update=pgd_update, grad_assemble=grad_assemble, image_grad=image_grad), null


@pytest.mark.parametrize("name", ["pgd_update", "grad_assemble", "image_grad"])
def test_abi_null_pointers_pf_and_dtype(name):
    calls, null = _callers()
    call = calls[name]
    for k in {"pgd_update": ("x", "x0"), "grad_assemble": ("x", "x0", "g"),
              "image_grad": ("rec", "t", "g")}[name]:
        call("null", **{k: null})
    call("pf must divide S", pf=0)
    call("pf must divide S", pf=-2)
    call("pf must divide S", pf=3)
    call("unsupported dtype", dtype=BAD_DTYPE)
    call("unsupported dtype", dtype=-1)


@pytest.mark.parametrize("name", ["pgd_update", "grad_assemble", "image_grad"])
def test_abi_cpad_below_3_with_g_vgg(name):
    """cpad < 3 with a VGG gradient: the kernel reads channel c < 3 of a cpad-wide pixel."""
    calls, _ = _callers()
    for cpad in (2, 1, 0, -8):
        calls[name]("cpad must be >= 3", cpad=cpad, dtype=BAD_DTYPE)


@pytest.mark.parametrize("name", ["pgd_update", "grad_assemble", "image_grad"])
def test_abi_n_and_s_out_of_range(name):
    calls, _ = _callers()
    call = calls[name]
    for N in (0, -3, 65536, 70000, 1 << 30):
        call("N must be in 1", N=N, dtype=BAD_DTYPE)
    for S in (0, -32, 16385, 1 << 20):
        call("S must be in 1", S=S, dtype=BAD_DTYPE)


@pytest.mark.parametrize("name", ["pgd_update", "grad_assemble"])
def test_abi_enc_res_with_g_enc(name):
    calls, _ = _callers()
    call = calls[name]
    call("enc_res must divide S", enc=5)
    call("enc_res must divide S", enc=64)
    call("enc_res must divide S", enc=-16, dtype=BAD_DTYPE)  # S % −16 == 0, but not a resolution
    if name == "pgd_update":
        # (mia_grad_assemble once evaluated S % enc_res before looking at enc_res: no 0 there)
        call("enc_res must divide S", enc=0)


def test_abi_pgd_update_lo_above_hi():
    calls, _ = _callers()
    calls["pgd_update"]("lo <= hi", lo=1.0, hi=-1.0, dtype=BAD_DTYPE)
    calls["pgd_update"]("lo <= hi", lo=float("nan"), dtype=BAD_DTYPE)


# ---- ops wrappers: refused on the host before a pointer is taken ---------------------------------
def _imgs(shape=(2, 3, 8, 8), dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (2, 1, 8, 8), (2, 3, 8, 6), (3, 8, 8), (2, 3, 64)])
def test_ops_pgd_update_and_image_grad_need_n3ss(shape):
    from gfa_amd import ops
    x = _imgs(shape)
    with pytest.raises(ValueError, match=r"\(N,3,S,S\)"):
        ops.pgd_update(x, x.clone(), None, None, 1, 8, 0.37, 0.03, 0.06)
    with pytest.raises(ValueError, match=r"\(N,3,S,S\)"):
        ops.image_grad(x, x.clone(), None, x.clone(), 1, 0.37)


def test_ops_pgd_update_and_image_grad_shape_checks():
    from gfa_amd import ops
    x = _imgs()
    for cpad in (1, 2):
        gv = torch.zeros(2, 8, 8, cpad)
        with pytest.raises(ValueError, match="at least 3"):
            ops.pgd_update(x, x.clone(), gv, None, 1, 8, 0.37, 0.03, 0.06)
        with pytest.raises(ValueError, match="at least 3"):
            ops.image_grad(x, x.clone(), gv, x.clone(), 1, 0.37)
    gv = torch.zeros(2, 4, 4, 8)
    for pf in (0, 3, -1):
        with pytest.raises(ValueError, match="pf must divide S"):
            ops.pgd_update(x, x.clone(), gv, None, pf, 8, 0.37, 0.03, 0.06)
        with pytest.raises(ValueError, match="pf must divide S"):
            ops.image_grad(x, x.clone(), gv, x.clone(), pf, 0.37)
    with pytest.raises(ValueError, match="g_vgg: shape"):  # pooled by 2, passed as pf = 1
        ops.pgd_update(x, x.clone(), gv, None, 1, 8, 0.37, 0.03, 0.06)
    with pytest.raises(ValueError, match="g_vgg: shape"):
        ops.image_grad(x, x.clone(), gv, x.clone(), 1, 0.37)
    with pytest.raises(ValueError, match=r"\(N,3,S,S\) fp32"):
        ops.pgd_update(x.double(), x.double(), None, None, 1, 8, 0.37, 0.03, 0.06)
    with pytest.raises(ValueError, match="x0"):
        ops.pgd_update(x, _imgs((1, 3, 8, 8)), None, None, 1, 8, 0.37, 0.03, 0.06)
