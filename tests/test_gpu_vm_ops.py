"""The device surface VM, operator family by operator family (needs an
MI355X): the programs and operands of tests/vm_ops.py through
RenderContext.debug_run_surface against the GML interpreter.
tests/test_vm_ops_ref.py asserts on the CPU what those cases reach."""
import numpy as np
import pytest

import go_raytracer_amd as rt
import vm_ops as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(V.PROGRAMS))
def test_device_vm_equals_the_interpreter(ctx, name):
    """Error flags equal; the ten outputs bit-equal where there is no error,
    any NaN equal to any NaN (registers after an error are outside the
    contract)."""
    ctx.set_scene(V.packed(name))
    cases = V.cases(name)
    out, err = ctx.debug_run_surface(0, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    want = V.expected(name)
    assert len(want) == len(cases) == len(err)
    werr = np.array([w is None for w in want])
    bad = np.flatnonzero((err != 0) != werr)
    assert len(bad) == 0, (name, "error flag", len(bad), cases[bad[0]], int(err[bad[0]]))
    ok = np.flatnonzero(~werr)
    assert len(ok) >= 50
    ref = np.array([want[k] for k in ok], dtype=np.float64)
    got = out[ok]
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    rows = np.flatnonzero(~same.all(axis=1))
    assert len(rows) == 0, (name, len(rows), cases[ok[rows[0]]], list(got[rows[0]]), list(ref[rows[0]]))
