"""The operator's ADMM entry points (csrc/operator_kernels.hip) and the float product refuse bad
arguments on the host, before any launch: -1 with revs_last_error() naming the entry.  No GPU: the
pointers handed over are never followed."""
import numpy as np
import pytest

import operator_cases as oc

GOOD = dict(n=4, m=4, T=8, nslab=1, kappa=5.0, alpha=1.6, vlo=-0.5, vhi=0.5, preclamp=0)
T_LIMIT = ("revs_op_home_pass", "revs_op_home_pass_fused", "revs_op_node_update", "revs_op_node_prep",
           "revs_op_node_apply", "revs_op_nodefast_update", "revs_op_nodefast_dualres")
ORDERED = ("revs_op_home_pass_fused", "revs_op_node_update", "revs_op_nodefast_update", "revs_op_nodefast_feas")


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()                     # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    return np.zeros(64)               # any non-null address: a refused call never reads it


def _refused(lib, buf, entry, **change):
    """Call `entry` with good arguments except `change` (scalar -> value, array name -> None)."""
    args = []
    for tok in oc.ARGS[entry]:
        name = tok.lstrip("@")
        val = change[name] if name in change else (buf.ctypes.data if tok[0] == "@" else GOOD[name])
        args.append(val)
    rc = getattr(lib, entry)(*args, None)
    err = lib.revs_last_error().decode()
    assert rc == -1 and err.startswith(entry + ":"), (entry, change, rc, err)
    return err


@pytest.mark.parametrize("entry", sorted(oc.ARGS))
def test_sizes_and_null_pointers(lib, buf, entry):
    size = "n" if "n" in oc.ARGS[entry] else "m"
    _refused(lib, buf, entry, **{size: 0})
    _refused(lib, buf, entry, **{size: -3})
    _refused(lib, buf, entry, T=0)
    required = [t[1:] for t in oc.ARGS[entry] if t[0] == "@" and t[1:] not in oc.OPTIONAL.get(entry, ())]
    assert len(required) >= 2
    for name in required:
        _refused(lib, buf, entry, **{name: None})
    if "nslab" in oc.ARGS[entry]:
        _refused(lib, buf, entry, nslab=0)
    if "kappa" in oc.ARGS[entry] and entry in ("revs_op_g0", "revs_op_node_prep", "revs_op_node_apply"):
        _refused(lib, buf, entry, kappa=0.0)


def test_every_entry_with_slabs_is_covered():
    with_slabs = {e for e, a in oc.ARGS.items() if "nslab" in a}
    assert with_slabs == {"revs_op_home_pass_fused", "revs_op_node_scale", "revs_op_node_update",
                          "revs_op_nodefast_scale", "revs_op_nodefast_update", "revs_op_nodefast_dualres",
                          "revs_op_nodefast_feas", "revs_op_nodefast_finish"}


@pytest.mark.parametrize("entry", T_LIMIT)
def test_more_than_256_slots(lib, buf, entry):
    _refused(lib, buf, entry, T=257)


@pytest.mark.parametrize("entry", ORDERED)
def test_bounds_out_of_order(lib, buf, entry):
    _refused(lib, buf, entry, vlo=0.5, vhi=-0.5)


def test_home_pass_residuals_need_cty_and_xc(lib, buf):
    assert "res needs" in _refused(lib, buf, "revs_op_home_pass", cty=None)
    assert "res needs" in _refused(lib, buf, "revs_op_home_pass", xc=None)


def test_float_product(lib, buf):
    p = buf.ctypes.data
    for args in ((4, 193, 4, p, 4, p, 193, p, 193, 0),        # more than 192 columns
                 (8, 4, 4, p, 7, p, 4, p, 4, 0),              # lda < m
                 (8, 4, 4, p, 8, p, 3, p, 4, 0),              # ldb < n
                 (8, 4, 4, p, 8, p, 4, p, 3, 0),              # ldc < n
                 (0, 4, 4, p, 8, p, 4, p, 4, 0), (8, 4, 0, p, 8, p, 4, p, 4, 0),
                 (8, 4, 4, None, 8, p, 4, p, 4, 0), (8, 4, 4, p, 8, None, 4, p, 4, 0),
                 (8, 4, 4, p, 8, p, 4, None, 4, 0)):
        rc = lib.revs_gemm_tn_f32(*args, None)
        assert rc == -1 and lib.revs_last_error().decode().startswith("revs_gemm_tn_f32:"), args
