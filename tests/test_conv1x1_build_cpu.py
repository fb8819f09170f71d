"""No GPU: the register edges of conv1x1.hip's kernel.  `conv1x1_ws_kernel<KST, ACT, SAT, COOP, ROW>` keeps the whole K of a wave's 32 filters
in registers (4 KST of them); its launch bounds promise four waves per SIMD (at most 128 registers) for KST <= 8 -- two eight-wave
workgroups per CU -- and, for the head form (ROW: one filter quad with a spare accumulator row), for KST = 16 as well, so that the small
workgroups the throughput plan gives the 512 -> 30 head share a CU.  Everything else runs two waves per SIMD (at most 256).  An
instantiation pushed over its edge spills into scratch memory -- silently, as far as the bytes go.  The numbers are read from the
`.amdhsa_*` metadata of the gfx950 assembly, compiled with the product flags (yolo_quantization_amd/csrc/build.sh)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "yolo_quantization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRODUCT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="needs hipcc to cross-compile to gfx950 assembly")

# private_segment_fixed_size of the (KST, ACT, SAT, COOP) instantiations at the commit before the ROW form: the twelve 64-channel ones
# spilled a few dwords at 128 registers (no net of BASELINE.json runs them); every other one had none.  ACT: 9 LEAKY, 8 RELU6, 3 LINEAR
SCRATCH_BEFORE = {(2, 9, 1, 1): 20, (2, 9, 1, 0): 20, (2, 9, 0, 1): 12, (2, 9, 0, 0): 20, (2, 8, 1, 1): 36, (2, 8, 1, 0): 44,
                  (2, 8, 0, 1): 20, (2, 8, 0, 0): 20, (2, 3, 1, 1): 36, (2, 3, 1, 0): 36, (2, 3, 0, 1): 36, (2, 3, 0, 0): 36}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "conv1x1.s")
    subprocess.check_call([HIPCC, *PRODUCT_FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "conv1x1.hip")], stderr=subprocess.DEVNULL)
    meta, key = {}, None
    for ln in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            k = re.fullmatch(r"_Z17conv1x1_ws_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])EEv8ConvArgs", m.group(1))
            key = tuple(int(v) for v in k.groups()) if k else None
            if key:
                meta[key] = {}
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)", ln)
        if m and key:
            meta[key][m.group(1)] = int(m.group(2))
    return meta


def test_every_instantiation_is_there(kernels):
    # five channel depths x three activations x two stores x (all waves sum / the wave sums / the sum row)
    want = {(kst, act, sat, coop, row) for kst in (2, 4, 8, 16, 32) for act in (9, 8, 3) for sat in (0, 1) for coop, row in ((1, 0), (0, 0), (0, 1))}
    assert set(kernels) == want, sorted(set(kernels) ^ want)


def test_register_limits(kernels):
    for (kst, act, sat, coop, row), v in kernels.items():
        limit = 128 if kst <= (16 if row else 8) else 256
        assert v["next_free_vgpr"] <= limit, ((kst, act, sat, coop, row), v)


def test_no_new_scratch(kernels):
    for (kst, act, sat, coop, row), v in kernels.items():
        before = 0 if row else SCRATCH_BEFORE.get((kst, act, sat, coop), 0)  # the ROW form is new: none at all
        assert v["private_segment_fixed_size"] <= before, ((kst, act, sat, coop, row), v, before)
