"""No GPU: the register edges and the K loop's LDS waits of the two row-image kernels (conv_rows.hip, conv_rows16.hip), 3x3 path.

Both kernels run two workgroups per CU at up to 256 registers; an instantiation pushed over what it had spills into scratch memory
(silently, as far as the bytes go) or loses the second wave of a SIMD.  The K loop hides its LDS latency behind hand-counted
`s_waitcnt lgkmcnt(n)` immediates: a full drain, `lgkmcnt(0)`, inside the steady-state chunk body is a wave that issues no MFMA while
its LDS queue empties, paid by the whole workgroup at the next barrier.  The numbers are read from the gfx950 assembly,
compiled with the product flags (yolo_quantization_amd/csrc/build.sh)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "yolo_quantization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRODUCT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
ROWS16_FLAGS = ["-mllvm", "-pragma-unroll-threshold=1000000"]  # build.sh, conv_rows16 only

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="needs hipcc to cross-compile to gfx950 assembly")

# (.amdhsa_next_free_vgpr, private_segment_fixed_size) of every 3x3 instantiation at the commit before the sums moved into registers.
# conv_rows16_i8_kernel<BM, BN, WMW, WNW, RS, 3, NBX>, keyed (BM, BN, RS, NBX):
ROWS16_BEFORE = {(128, 384, 16, 0): (256, 24), (128, 256, 16, 0): (191, 0), (128, 192, 16, 0): (246, 0), (128, 128, 16, 0): (172, 0),
                 (64, 256, 16, 0): (176, 0), (64, 128, 16, 0): (108, 0), (128, 384, 32, 4): (256, 44)}
# conv_rows_i8_kernel<BM, BN, WMW, WNW, RS, 3>, keyed (BM, BN, RS): no scratch anywhere
ROWS_BEFORE = {(128, 384, 16): 214, (128, 256, 16): 161, (128, 192, 16): 210, (128, 128, 16): 154, (64, 256, 16): 160, (64, 128, 16): 96,
               (32, 256, 16): 111, (32, 128, 16): 104,
               (128, 384, 32): 214, (128, 256, 32): 161, (128, 192, 32): 210, (128, 128, 32): 154, (64, 256, 32): 162, (64, 128, 32): 96,
               (32, 256, 32): 112, (32, 128, 32): 100,
               (128, 384, 64): 217, (128, 256, 64): 165, (128, 192, 64): 212, (128, 128, 64): 158, (64, 256, 64): 164, (64, 128, 64): 98,
               (32, 256, 64): 114, (32, 128, 64): 102}

# Instantiations whose K loop keeps sum(x') in registers and counts its cell reads (conv_rows16.hip where a thread owns
# one cell) -> the `s_waitcnt lgkmcnt(0)` their chunk loop may hold between its first and last MFMA.  None -- except for the 32-column
# wave tiles of 64 x 128: there the fragment pipeline's own mid-step wait, `lgkmcnt(NI - 2)` with NI = 2, is spelled lgkmcnt(0) in
# each of the eight K-steps behind the first MFMA (two fragment reads in flight, as in every other instantiation); the parent had twelve.
ROWS16_COUNTED = {(128, 256, 16, 0): 0, (128, 128, 16, 0): 0, (64, 128, 16, 0): 8}
ROWS_COUNTED = {}  # conv_rows.hip keeps the per-chunk call: the counted form costs it registers


def _compile_all(tmp):
    """both translation units at once (each takes a minute or two) -> {name: path of its assembly}"""
    jobs = {}
    for name, extra in (("conv_rows16", ROWS16_FLAGS), ("conv_rows", [])):
        out = os.path.join(tmp, name + ".s")
        jobs[name] = (out, subprocess.Popen([HIPCC, *PRODUCT_FLAGS, *extra, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, name + ".hip")],
                                            stderr=subprocess.DEVNULL))
    for name, (out, p) in jobs.items():
        assert p.wait() == 0, name
    return {name: out for name, (out, _) in jobs.items()}


def _parse(path, pattern):
    """-> {key: {"next_free_vgpr", "private_segment_fixed_size", "body": [instruction lines]}} of the kernels whose symbol matches"""
    meta, key, sym_key, body = {}, None, {}, None
    for ln in open(path):
        m = re.match(r"(_Z\w+):\s*(;.*)?$", ln)
        if m:  # function label: the body runs to s_endpgm
            k = re.fullmatch(pattern, m.group(1))
            body = None
            if k:
                sym_key[m.group(1)] = tuple(int(v) for v in k.groups())
                body = meta.setdefault(sym_key[m.group(1)], {}).setdefault("body", [])
            continue
        if body is not None:
            body.append(ln.strip())
            if ln.strip().startswith("s_endpgm"):
                body = None
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            key = sym_key.get(m.group(1))
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)", ln)
        if m and key:
            meta[key][m.group(1)] = int(m.group(2))
    return meta


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return _compile_all(str(tmp_path_factory.mktemp("asm")))


@pytest.fixture(scope="module")
def rows16(asm):
    return _parse(asm["conv_rows16"], r"_Z21conv_rows16_i8_kernelILi(\d+)ELi(\d+)ELi\d+ELi\d+ELi(\d+)ELi3ELi(\d+)EEv8ConvArgs")


@pytest.fixture(scope="module")
def rows(asm):
    return _parse(asm["conv_rows"], r"_Z19conv_rows_i8_kernelILi(\d+)ELi(\d+)ELi\d+ELi\d+ELi(\d+)ELi3EEv8ConvArgs")


def chunk_loop(body):
    """the steady-state chunk loop: the largest span from a label to a backward branch to it that holds MFMAs -> its instruction lines"""
    labels = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    best = []
    for i, ln in enumerate(body):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", ln) or re.match(r"s_branch\s+(\.LBB\d+_\d+)", ln)
        if m and labels.get(m.group(1), i) < i:
            span = body[labels[m.group(1)]:i + 1]
            if sum("v_mfma" in s for s in span) > sum("v_mfma" in s for s in best):
                best = span
    return best


def drains_between_mfmas(loop):
    at = [i for i, s in enumerate(loop) if s.startswith("v_mfma")]
    return [s for s in loop[at[0]:at[-1]] if s.startswith("s_waitcnt") and re.search(r"lgkmcnt\(0\)", s)]


def test_every_3x3_instantiation_is_there(rows16, rows):
    assert set(rows16) == set(ROWS16_BEFORE), sorted(set(rows16) ^ set(ROWS16_BEFORE))
    assert set(rows) == set(ROWS_BEFORE), sorted(set(rows) ^ set(ROWS_BEFORE))


def test_rows16_registers_and_scratch(rows16):
    for key, (vgpr, scratch) in ROWS16_BEFORE.items():
        v = rows16[key]
        assert v["next_free_vgpr"] <= vgpr and v["private_segment_fixed_size"] <= scratch, (key, v["next_free_vgpr"], v["private_segment_fixed_size"], vgpr, scratch)


def test_rows_registers_and_scratch(rows):
    for key, vgpr in ROWS_BEFORE.items():
        v = rows[key]
        assert v["next_free_vgpr"] <= vgpr and v["private_segment_fixed_size"] == 0, (key, v["next_free_vgpr"], v["private_segment_fixed_size"], vgpr)


def test_chunk_loop_is_found(rows16, rows):
    """the loop finder sees nine K-steps of MFMAs in every instantiation (so that the drain test below looks at the right span)"""
    for key, v in rows16.items():
        bm, bn = key[0], key[1]
        nw = 8 if bn >= 256 and bm == 128 else 4
        per_step = (bm // 16) * (bn // 16) // nw  # 16 x 16 x 64 MFMAs of one wave per K-step
        assert sum(s.startswith("v_mfma") for s in chunk_loop(v["body"])) == 9 * per_step, key
    for key, v in rows.items():
        bm, bn = key[0], key[1]
        nw = 8 if bn >= 256 and bm == 128 else 4
        per_step = 2 * (bm // 32) * (bn // 32) // nw  # 32 x 32 x 32 MFMAs: two k-halves
        assert sum(s.startswith("v_mfma") for s in chunk_loop(v["body"])) == 9 * per_step, key


def test_counted_chunk_loops_do_not_drain_lds(rows16, rows):
    for key, allowed in sorted(ROWS16_COUNTED.items()):
        assert len(drains_between_mfmas(chunk_loop(rows16[key]["body"]))) == allowed, ("conv_rows16", key)
    for key, allowed in sorted(ROWS_COUNTED.items()):
        assert len(drains_between_mfmas(chunk_loop(rows[key]["body"]))) == allowed, ("conv_rows", key)


def test_loop_finder_sees_the_drains_of_the_uncounted_form(rows16, rows):
    """an instantiation that keeps the per-chunk cell_sums call drains its queue around it: the finder must see that"""
    for key in sorted(set(rows16) - set(ROWS16_COUNTED)):
        assert len(drains_between_mfmas(chunk_loop(rows16[key]["body"]))) >= 2, ("conv_rows16", key)
    for key in sorted(set(rows) - set(ROWS_COUNTED)):
        assert len(drains_between_mfmas(chunk_loop(rows[key]["body"]))) >= 2, ("conv_rows", key)


def _vgprs(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def lds_hazards(body):
    """Walk the kernel in program order with a model of the in-order LDS return queue: `s_waitcnt lgkmcnt(n)` retires all but the n
    youngest operations; an instruction between the first and the last MFMA that touches a register which an outstanding ds_read
    still has to write reads it too early (or overwrites what the read will overwrite) -> [(instruction, the read)]"""
    at = [i for i, s in enumerate(body) if s.startswith("v_mfma")]
    queue, bad = [], []
    for i, ln in enumerate(body[:at[-1] + 1]):
        ln = ln.split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        op = ln.split()[0]
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", ln)
            if m and len(queue) > int(m.group(1)):
                queue = queue[len(queue) - int(m.group(1)):] if int(m.group(1)) else []
            continue
        touched = _vgprs(ln[len(op):])
        if i >= at[0]:
            bad += [(ln, rd) for dst, rd in queue if dst & touched]
        if op.startswith("ds_read"):
            queue.append((_vgprs(ln[len(op):].split(",")[0]), ln))
        elif op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
            queue.append((set(), ln))
    return bad


def test_counted_waits_cover_every_read(rows16, rows):
    """the hand-counted immediates: no MFMA or v_dot4 of a K loop consumes a fragment or a cell piece that may still be in flight"""
    for name, kernels in (("conv_rows16", rows16), ("conv_rows", rows)):
        for key, v in kernels.items():
            bad = lds_hazards(v["body"])
            assert not bad, (name, key, bad[:3])


def test_the_hazard_walk_sees_a_loosened_wait(rows16):
    """the same walk on the 128 x 128 kernel with every lgkmcnt(2) loosened to 3 must find consumers of reads in flight"""
    body = [ln.replace("lgkmcnt(2)", "lgkmcnt(3)") for ln in rows16[(128, 128, 16, 0)]["body"]]
    assert lds_hazards(body)
