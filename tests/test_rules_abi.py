"""revs_rule_schedule (include/revs_admm_ops.h) is declared, exported and bound, and bad arguments are rejected on the
host, before any launch, with a message that names the argument (no GPU here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from revs_admm_amd import _lib, build
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_rule_schedule\s*\(", ops)
    assert "revs_rule_schedule" not in boundary                  # (the boundary header stays at its 45 functions)
    assert hasattr(lib, "revs_rule_schedule")
    assert len(_lib.SIGNATURES["revs_rule_schedule"][1]) == 12
    assert "rule_kernels.hip" in build.SOURCES
    for name, value in (("REVS_RULE_ASAP", 0), ("REVS_RULE_ALAP", 1), ("REVS_RULE_EVEN", 2), ("REVS_FILL_TARGET", 0),
                        ("REVS_FILL_FULL", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", ops), name
    assert (_lib.RULE_ASAP, _lib.RULE_ALAP, _lib.RULE_EVEN, _lib.FILL_TARGET, _lib.FILL_FULL) == (0, 1, 2, 0, 1)
    from revs_admm_amd import baselines
    assert baselines.POLICIES == dict(uncontrolled=0, last_minute=1, trickle=2)


def _call(lib, rows=8, T=24, homes=64, load=128, policy=0, fill=0, integral=1, p=256, soc=512, g=1024, status=2048):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    return lib.revs_rule_schedule(rows, T, homes, load, policy, fill, integral, p, soc, g, status, None)


def test_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    for rows in (0, -1, -2 ** 40):
        assert _call(lib, rows=rows) == -1 and f"revs_rule_schedule: rows={rows}".encode() in err()
    assert _call(lib, rows=2 ** 45) == -1 and b"rows=" in err()
    for T in (0, -1, 193):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in err()
    assert _call(lib, homes=None) == -1 and b"argument homes" in err()
    for policy in (-1, 3, 99):
        assert _call(lib, policy=policy, integral=0) == -1 and f"policy={policy}".encode() in err()
    for fill in (-1, 2):
        assert _call(lib, fill=fill) == -1 and f"fill={fill}".encode() in err()
    for integral in (1, 2, -1):
        assert _call(lib, policy=2, integral=integral) == -1
        assert b"REVS_RULE_EVEN" in err() and f"integral={integral}".encode() in err()
    assert _call(lib, p=None, soc=None, g=None, status=None) == -1 and b"every output is NULL" in err()
    for name in (b"p_out", b"soc_out", b"g_out", b"status_out"):
        assert name in err()
    assert _call(lib, load=None) == -1 and b"g_out without load" in err()
    assert _call(lib, load=None, p=None, soc=None, status=None) == -1 and b"g_out without load" in err()


def test_python_layer_refuses_before_the_device():
    from revs_admm_amd import baselines
    import numpy as np
    from revs_admm_amd._lib import HOME_DTYPE
    homes, load = np.zeros(3, HOME_DTYPE), np.zeros((3, 24), np.float32)
    with pytest.raises(ValueError, match="trickle"):
        baselines.rule_schedule(homes, load, policy="trickle", charger="binary")
    with pytest.raises(ValueError, match="policy must be"):
        baselines.rule_schedule(homes, load, policy="centralized")
    with pytest.raises(ValueError, match="fill must be"):
        baselines.rule_schedule(homes, load, fill="half")
    with pytest.raises(ValueError, match="charger must be"):
        baselines.rule_schedule(homes, load, charger="fast")
    assert baselines.rule_args("trickle", "full", "relaxed_exact") == (2, 1, 0)
    assert baselines.rule_args("last_minute", "target", "binary") == (1, 0, 1)
    assert baselines.rule_args("uncontrolled", "target", 0) == (0, 0, 1) and baselines.rule_args("trickle", "full", 2)[2] == 0
