"""The train step's four persistent-kernel files on the one staged tile (csrc/train_tile.h), checked without a GPU: what the
compiler makes of each of their 29 instantiations, against the figures of the listing before the tile moved into the header
(the four files then each carried their own copy of the pipeline): the same LDS, scratch and spills, no more registers, and the same
ordered sequence of matrix, LDS, global-memory and barrier instructions.  Listing, figures and sequence are those of
profiles/train_tile_listing.py, which prints the full comparison of two trees.  Also: the matrix instruction and the cell's
pointwise backward are each written in one place."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc')
HIPCC = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'

_spec = importlib.util.spec_from_file_location('train_tile_listing', os.path.join(ROOT, 'profiles', 'train_tile_listing.py'))
tl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tl)

# kernel: (VGPRs + AGPRs, LDS bytes, scratch bytes, VGPR spills, SGPR spills, sha256[:16] of the ordered sequence without waits),
# recorded from the listing of the commit before train_tile.h (hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S)
PARENT = {
    'train_persist.hip': {
        'train_recurrence_kernel<1>': (132, 46084, 0, 0, 0, 'd1a70bc741be16e9'),
        'train_recurrence_kernel<2>': (124, 46084, 0, 0, 0, '9f8bf70568576f9f'),
        'train_recurrence_kernel<3>': (136, 46084, 0, 0, 0, 'ee974732ef5755d1'),
        'train_recurrence_kernel<4>': (156, 46084, 0, 0, 0, '966dfd7c36249aba'),
        'train_recurrence_kernel<5>': (160, 46084, 0, 0, 0, 'fc76930980224d1e'),
        'train_recurrence_kernel<6>': (162, 46084, 0, 0, 0, '4690a2a6966df0d6'),
        'train_recurrence_kernel<7>': (166, 46084, 0, 0, 0, '8bf72f2c1615b648'),
        'train_recurrence_kernel<8>': (168, 46084, 0, 0, 0, '587ab90ae1b6d3b8'),
        'train_recurrence_kernel<9>': (174, 46084, 0, 0, 0, 'ade3de5d21f0daf6'),
        'train_recurrence_kernel<10>': (178, 46084, 0, 0, 0, '6afee0182dc524a6'),
        'train_recurrence_kernel<11>': (182, 46084, 0, 0, 0, 'f85971466daf2c10'),
        'train_recurrence_kernel<12>': (186, 46084, 0, 0, 0, 'e4e5f025f405d81b'),
        'train_recurrence_kernel<13>': (190, 46084, 0, 0, 0, '3c536bbee67114ae'),
        'train_recurrence_kernel<14>': (194, 46084, 0, 0, 0, '7c75dc179b09a153'),
        'train_recurrence_kernel<15>': (198, 46084, 0, 0, 0, '606a878c1f34ce94'),
        'train_recurrence_kernel<16>': (202, 46084, 0, 0, 0, '982288ee62727302'),
    },
    'train_persist_bwd.hip': {
        'train_recurrence_bwd_kernel<4>': (176, 46084, 0, 0, 0, '7b2d11e620bd364e'),
        'train_recurrence_bwd_kernel<8>': (192, 46084, 0, 0, 0, '34f0e52e140477ee'),
        'train_recurrence_bwd_kernel<12>': (206, 46084, 0, 0, 0, 'aa8be33e6b2a0d32'),
        'train_recurrence_bwd_kernel<16>': (224, 46084, 0, 0, 0, 'bd339214d31ea49e'),
    },
    'train_persist_top.hip': {
        'train_attention_cell_kernel<4>': (260, 55300, 0, 0, 118, 'd04bd6ab9aa69b2c'),
        'train_attention_cell_kernel<8>': (412, 55300, 0, 0, 75, '377ffc7d30b02291'),
        'train_attention_cell_kernel<16>': (348, 55300, 0, 0, 44, '6b2422e2f8cce161'),
    },
    'train_persist_topb.hip': {
        'train_attention_cell_bwd_kernel<4>': (292, 46084, 0, 0, 111, '1b5d140202e8062c'),
        'train_attention_cell_bwd_kernel<8>': (292, 46084, 0, 0, 118, '7df5f64ddd6b4d8e'),
        'train_attention_cell_bwd_kernel<16>': (324, 46084, 0, 0, 89, '985ae185d742a380'),
        'train_attention_cell_bwd_rows_kernel<4>': (141, 8708, 0, 0, 44, '208e92e371b8cb16'),
        'train_attention_cell_bwd_rows_kernel<8>': (133, 8708, 0, 0, 46, '82e2def9b8663f0f'),
        'train_attention_cell_bwd_rows_kernel<16>': (168, 8708, 20, 4, 9, 'ec1e3ef4de1f2175'),
    },
}


def test_the_table_lists_the_29_instantiations():
    assert list(PARENT) == tl.FILES and [len(v) for v in PARENT.values()] == [16, 4, 3, 6]


@pytest.mark.parametrize('name', tl.FILES)
def test_each_instantiation_keeps_its_figures_and_its_ordered_sequence(name, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc on this box')
    text = tl.listing(ROOT, name, str(tmp_path))
    kernels, figures = tl.kernels(text), tl.figures(text)
    assert sorted(kernels) == sorted(figures) == sorted(PARENT[name])
    for kernel, (regs, lds, scratch, vspill, sspill, digest) in PARENT[name].items():
        f = figures[kernel]
        print(kernel, f, tl.sequence_digest(kernels[kernel]))
        assert (f['group_segment_fixed_size'], f['private_segment_fixed_size'], f['vgpr_spill_count'], f['sgpr_spill_count']) \
            == (lds, scratch, vspill, sspill), kernel
        assert f['vgpr_count'] + f['agpr_count'] <= regs, kernel
        assert tl.sequence_digest(kernels[kernel]) == digest, kernel + ': the ordered sequence of matrix, LDS, memory and barrier instructions moved'


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_matrix_instruction_and_the_cell_backward_are_written_once():
    for name in tl.FILES:
        assert 'mfma_f32_32x32x2f32' not in _src(name), name
    assert 'mfma_f32_32x32x2f32' in _src('train_tile.h')
    sources = {n: _src(n) for n in os.listdir(CSRC) if n.endswith(('.hip', '.h'))}
    assert sum(s.count('LstmCellBwdOut lstm_cell_bwd(') for s in sources.values()) == 1 == sources['common.h'].count('LstmCellBwdOut lstm_cell_bwd(')
    assert [n for n, s in sources.items() if '(1.0f - gg * gg)' in s] == ['common.h']
    for name in ('train_kernels.hip', 'gemm_bwd.hip', 'train_persist_bwd.hip', 'train_persist_topb.hip'):
        assert 'lstm_cell_bwd(' in sources[name], name
