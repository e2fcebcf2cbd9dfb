"""The device code of icp_hip.hip as assembly, compiled once per test process with the product's own flags; the register-budget tests
of every feature read the counts the compiler reports from it.  No GPU needed."""
import functools
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@functools.lru_cache(maxsize=None)
def device_asm():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-Wall")]      # the product's own flags
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "icp-variants_amd", "csrc", "icp_hip.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "icp_hip.s")
        subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-w", "-I", os.path.join(ROOT, "include"), "-S", src, "-o", out], timeout=900)
        with open(out) as f:
            return f.read()


def kernel_resources(text):
    """{symbol: {"num_vgpr": .., "num_agpr": .., "private_seg_size": ..}} of every icpdev symbol, from the assembly's .set lines."""
    seen = {}
    for name, field, val in re.findall(r"\.set (_ZN6icpdev\S*?)\.(num_vgpr|num_agpr|private_seg_size), (\d+)", text):
        seen.setdefault(name, {})[field] = int(val)
    return seen
