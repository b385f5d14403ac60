"""What the test-side helpers of the screen passes (tests/<pass>_ref.py) share: building a small C++ program of
tests/native/ with the restatements' flags, the in.bin / out.bin round trip through one, and the fp16 bit-pattern helpers
the inputs are made with.  The arithmetic the restatements themselves share is tests/native/ref_contract.h."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import __graft_entry__ as g

f32 = np.float32
NATIVE_DIR = os.path.join(g.ROOT, "tests", "native")
FLAGS = ("-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math")  # one IEEE operation per operation, std::fma the only fused one
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@functools.lru_cache(maxsize=None)
def _exe_dir():
    d = tempfile.mkdtemp(prefix="native_ref_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def build(name, *, include=(), extra=(), sanitize=False):
    """compile tests/native/<name>.cpp (or, with a path, that source) -> the executable's path.  include: -I directories;
    extra: further flags, after the restatements' own; sanitize: with the address and undefined-behaviour sanitizers (a
    stand-alone program, run directly)"""
    src = name if os.sep in str(name) else os.path.join(NATIVE_DIR, name + ".cpp")
    exe = os.path.join(tempfile.mkdtemp(dir=_exe_dir()), os.path.splitext(os.path.basename(src))[0])
    flags = [*FLAGS, *extra, *(SANITIZE if sanitize else ())]
    for d in include:
        flags += ["-I", str(d)]
    subprocess.run(["g++", *flags, "-o", exe, str(src)], check=True)
    return exe


def run(exe, blob, *mode):
    """exe [mode ...] in.bin out.bin over blob -> out.bin's bytes"""
    with tempfile.TemporaryDirectory(prefix="native_ref_io_") as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        subprocess.run([exe, *mode, fin, fout], check=True)
        with open(fout, "rb") as f:
            return f.read()


def halves(values):
    """float array -> fp16 bit patterns (numpy's cast; for building inputs)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(values, dtype=f32).astype(np.float16).view(np.uint16)


def floats(bits):
    """fp16 bit patterns -> float32, exactly (signalling NaNs among them: numpy reports those as invalid)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(f32)


def san_bits(bits):
    """san as the bit operation on halves it is (C62): NaN, negatives and -0 become 0, +inf the largest half"""
    bits = np.asarray(bits, np.uint16)
    out = bits.copy()
    out[bits >= 0x7c00] = 0
    out[bits == 0x7c00] = 0x7bff
    return out


# the halves a colour target can hold that are no ordinary colour: NaNs, +-inf, negatives, -0, 65504, subnormals, 0; and 1
SPECIALS = np.array([0x7e00, 0xfe00, 0x7c01, 0x7c00, 0xfc00, 0xbc00, 0xc500, 0x8000, 0x7bff, 0x0001, 0x03ff, 0x8001, 0x0000, 0x3c00], np.uint16)
