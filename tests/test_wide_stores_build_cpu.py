"""No GPU: the register edges of the two kernels whose epilogues exchange their packed dwords across lanes for one wide store per tile.
conv_first_mfma_pool_kernel with 16 filters runs four waves per SIMD (at most 128 VGPRs), conv_pool16_kernel three (at most 168); an
instantiation pushed over its edge halves its occupancy or spills into scratch memory -- silently, as far as the bytes go.  The limits are
read from the `.amdhsa_*` metadata of the gfx950 assembly, compiled with the product flags (yolo_quantization_amd/csrc/build.sh)."""
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

# private_segment_fixed_size at the commit before the wide stores: "no scratch where there was none" (every other instantiation below had 0)
P16_SCRATCH_BEFORE = {"_Z18conv_pool16_kernelILi9ELb1EEv8ConvArgs": 20}                       # LEAKY, saturating store
L0_SCRATCH_BEFORE = {"_Z27conv_first_mfma_pool_kernelILi9ELb0ELi1ELb0ELb1EEv7AuxArgs": 20}    # LEAKY, wrap, cell input, per-image


def _metadata(src, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / (src + ".s"))
    subprocess.check_call([HIPCC, *PRODUCT_FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)], stderr=subprocess.DEVNULL)
    meta, name = {}, None
    for ln in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            name = m.group(1)
            meta[name] = {}
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)", ln)
        if m and name:
            meta[name][m.group(1)] = int(m.group(2))
    return meta


@pytest.fixture(scope="module")
def pool16_meta(tmp_path_factory):
    return _metadata("conv_pool16.hip", tmp_path_factory)


@pytest.fixture(scope="module")
def aux_meta(tmp_path_factory):
    return _metadata("conv_aux.hip", tmp_path_factory)


def test_conv_pool16_stays_at_three_waves_per_simd(pool16_meta):
    ks = {k: v for k, v in pool16_meta.items() if "conv_pool16_kernel" in k}
    assert len(ks) == 6, sorted(ks)  # LEAKY / RELU6 / LINEAR x wrap / saturate
    for k, v in ks.items():
        assert v["next_free_vgpr"] <= 168, (k, v)
        if P16_SCRATCH_BEFORE.get(k, 0) == 0:
            assert v["private_segment_fixed_size"] == 0, (k, v)


def test_first_layer_pool_16_filters_stays_at_four_waves_per_simd(aux_meta):
    ks = {k: v for k, v in aux_meta.items() if re.search(r"conv_first_mfma_pool_kernelILi\dELb[01]ELi1E", k)}
    assert len(ks) == 24, sorted(ks)  # three activations x two stores x planar / cell x shared / per-image
    for k, v in ks.items():
        assert v["next_free_vgpr"] <= 128, (k, v)
        if L0_SCRATCH_BEFORE.get(k, 0) == 0:
            assert v["private_segment_fixed_size"] == 0, (k, v)
