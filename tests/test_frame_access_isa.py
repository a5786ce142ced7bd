"""The frame stack's memory instructions in the compiled render kernel (no
device needed): the C3 specialisation is compiled offline as hipRTC builds it
at run time (scripts/spec_regs.sh) and its listing is read.

The per-lane frame stack is split at run time: the cores of the shallow
levels in LDS, everything else in HBM (rt_render.h, core_load / core_store).
Both sides are typed by address space, so no access may be a FLAT one -- a
FLAT access needs a 64-bit address select per field, and it counts on vmcnt
and lgkmcnt both, so an LDS frame read would wait for the wave's HBM stores.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C3_KEY = ["-DRT_SPEC_KMASK=15", "-DRT_SPEC_FEAT=0", "-DRT_SPEC_NOBJ=4", "-DRT_SPEC_KINDS=1,3,2,0",
          "-DRT_SPEC_NLIGHTS=4", "-DRT_SPEC_POWBITS=6"]


def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    return None


@pytest.fixture(scope="module")
def c3_listing(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("frame_isa")
    src = d / "spec.hip"
    src.write_text('#include "rt_render.h"\n'
                   "template __global__ void rt_render_kernel<true, false, false, false>(const char*, Params);\n")
    out = d / "spec.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "go-raytracer_amd", "csrc"),
                        "--cuda-device-only", "-S", "-o", str(out), str(src)] + C3_KEY,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def kernel_body(listing):
    """The instructions of rt_render_kernel: from its label to its s_endpgm."""
    m = re.search(r"^(_Z16rt_render_kernel\w*):[^\n]*\n(.*?)^\s+s_endpgm", listing, re.M | re.S)
    assert m, "rt_render_kernel not found in the listing"
    return m.group(2)


def test_c3_frame_accesses_are_not_flat(c3_listing):
    body = kernel_body(c3_listing)
    flat = re.findall(r"^\s+(flat_(?:load|store)\w*)", body, re.M)
    assert not flat, "%d FLAT accesses in rt_render_kernel: %s" % (len(flat), sorted(set(flat)))
    # the two sides are there: LDS frame cores (rows 512 B apart) and HBM frames
    assert re.search(r"^\s+ds_read2st64_b64", body, re.M)
    assert re.search(r"^\s+global_load_dwordx2", body, re.M)


def test_c3_kernel_spills_no_vector_registers(c3_listing):
    m = re.search(r"^\s+\.vgpr_spill_count:\s*(\d+)", c3_listing, re.M)
    assert m, "no .vgpr_spill_count in the listing"
    assert int(m.group(1)) == 0
