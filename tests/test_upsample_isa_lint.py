"""ISA lint (CPU, needs only hipcc): the folded upsample conv (conv3x3_up2.hip) keeps its 32 accumulator tiles and 12 halo fragments in
registers -- no private segment (no scratch, so no spill) and at most 256 VGPRs (two workgroups per CU) in every instantiation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def test_folded_upsample_conv_does_not_spill(tmp_path):
    out = tmp_path / "conv3x3_up2.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "conv3x3_up2.hip")],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    blocks, cur = [], None
    for l in out.read_text().split("\n"):
        if re.match(r"^\s+- \.\w+:", l):              # a new list item of amdhsa.kernels (or of .args: those carry no .name)
            cur = {}; blocks.append(cur)
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    kernels = {b["name"]: b for b in blocks if "name" in b and "vgpr_count" in b}
    conv = {k: b for k, b in kernels.items() if "conv3x3_up2_kernel" in k}
    assert len(conv) == 2, sorted(kernels)                   # the bf16 and the fp16 operand form
    for k, b in kernels.items():
        assert int(b["private_segment_fixed_size"]) == 0, (k, b["private_segment_fixed_size"])
        assert int(b["vgpr_spill_count"]) == 0 and int(b["sgpr_spill_count"]) == 0, k
    for k, b in conv.items():
        assert int(b["vgpr_count"]) <= 256, (k, b["vgpr_count"])
