"""Emulator of the device surface VM with the contest-extension opcodes
(include/rt_abi.h RT_VM_EXT_ASIN / _ACOS / _REAL) -- test infrastructure.

Base instructions are run by tests/vm_emu.py. Programs are straight-line, so
an extension instruction is resolved in program order: its operand is read by
running the program up to it (vm_emu), its result is computed here, and the
instruction is replaced by a CONST of that result. The program that remains
holds base opcodes only and is run by vm_emu once more for the outputs and
the error flag."""
from go_raytracer_amd import gomath
from go_raytracer_amd.gml.evaluator import RAD_TO_DEG
from go_raytracer_amd.gml.surface_compiler import EXT_OPS, OP, OPS

import vm_emu
from vm_emu import b2f, b2i, f2b  # noqa: F401

_EXT = {OP[n]: n for n in EXT_OPS}
assert min(_EXT) == len(OPS)
# vm_emu hands a register back as a float: the operand's bits (an int64 for
# REAL) must survive that, signalling-NaN patterns included. They do where a
# float is moved and never computed with (struct copies the 8 bytes); stop
# loudly on a platform where they would not.
for _pattern in (0x7FF0000000000001, 0xFFF0000000000001, 0xFFFFFFFFFFFFFFFD, 0x7FF8000000000001):
    assert f2b(b2f(_pattern)) == _pattern, hex(_pattern)


def _ext_value(name, bits):
    if name == "ASIN":
        return f2b(RAD_TO_DEG * gomath.go_asin(b2f(bits)))
    if name == "ACOS":
        return f2b(RAD_TO_DEG * gomath.go_acos(b2f(bits)))
    if name == "REAL":
        return f2b(float(b2i(bits)))  # int -> float64 rounds to nearest even, as Go's float64(int64)
    raise ValueError(name)


def run(words, consts, face, u, v):
    """(10 material fields, error flag), like vm_emu.run."""
    words = list(words)
    consts = list(consts)
    for pc in range(0, len(words), 2):
        op = words[pc] & 0xFF
        if op == OP["RET"]:
            break
        if op not in _EXT:
            continue
        d, a = (words[pc] >> 8) & 0xFF, (words[pc] >> 16) & 0xFF
        # the operand: run the (already base-only) instructions before this one, then r0 = r[a]
        probe = words[:pc] + [OP["MOV"] | (0 << 8) | (a << 16), 0, OP["RET"], 0]
        out, _ = vm_emu.run(probe, consts, face, u, v)
        consts.append(_ext_value(_EXT[op], f2b(out[0])))
        words[pc] = OP["CONST"] | (d << 8)
        words[pc + 1] = len(consts) - 1
    return vm_emu.run(words, consts, face, u, v)
