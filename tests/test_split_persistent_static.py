"""The split arithmetic's persistent encoder (csrc/persist_split.hip), checked without a GPU: its gfx950 code object uses no
scratch memory and contracts on v_mfma_f32_32x32x16_bf16 alone (the 16x16 bf16 shapes sum in another order: their results would
not be the per-step launches' bits), and the public header documents what the option and the statistic now mean."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc')
HIPCC = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.fixture(scope='module')
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc on this box')
    out = str(tmp_path_factory.mktemp('asm') / 'persist_split.s')
    # (the flags of csrc/Makefile; device code only, as csrc/check_asm_loads.py obtains its listing)
    subprocess.run([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', '-o', out,
                    os.path.join(CSRC, 'persist_split.hip')], check=True, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    with open(out) as f:
        return f.read()


def test_kernel_is_built_with_the_library():
    with open(os.path.join(CSRC, 'Makefile')) as f:
        srcs = [ln for ln in f if ln.startswith('SRCS')][0]
    assert 'persist_split.hip' in srcs.split()


def test_no_scratch_and_only_the_32x32x16_bf16_instruction(listing):
    meta = listing[listing.index('amdhsa.kernels'):]
    kernels = re.findall(r'\.name:\s+(\S*persist_split_encode_kernel\S*)', meta)
    assert kernels, 'kernel metadata not found'
    blocks = [b for b in re.split(r'\n  - \.agpr_count', meta) if 'persist_split_encode_kernel' in b]
    assert len(blocks) == 1
    assert re.search(r'\.private_segment_fixed_size:\s+0\b', blocks[0]), 'the kernel uses scratch memory'
    assert re.search(r'\.vgpr_spill_count:\s+0\b', blocks[0]) and re.search(r'\.sgpr_spill_count:\s+0\b', blocks[0])
    assert 'v_mfma_f32_32x32x16_bf16' in listing
    assert not re.search(r'v_mfma_f32_16x16x\d+_bf16', listing), 'a 16x16 bf16 shape: another summation order'
    assert not re.search(r'v_mfma_f32_32x32x(?!16_bf16)\w+', listing), 'another 32x32 matrix instruction'


def test_header_documents_the_option_and_the_statistic():
    with open(os.path.join(ROOT, 'include', 'cor_asv_ann_hip.h')) as f:
        text = ' '.join(f.read().replace(' * ', ' ').split())
    assert 'persistent small-batch kernels (fp32-input kernels) are not used' not in text
    opt = text[text.index('"persistent" ='):text.index('"fused_backward" =')]
    assert 'persist_split.hip' in opt and 'ENCODER' in opt
    arith = text[text.index('"arithmetic" (per handle'):text.index('"split_bf16" (process-wide')]
    assert 'persist_split.hip' in arith and 'not used' not in arith
    stat = text[text.index('Statistics of the last call'):text.index('int casv_get_stat')]
    assert '"encoder_persistent"' in stat
