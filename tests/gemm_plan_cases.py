"""Inputs of the GEMM launch planner (cor_asv_ann_amd/csrc/gemm_plan.h) and the launches they become.

A case is one line for tests/gemm_plan_driver.cpp: `G name keys ; job keys ; job keys ...` for a batch of forward contractions,
`T name keys` for a weight-gradient contraction.  Keys left out take the driver's defaults (256 CUs, arithmetic 0, every switch at
its default, one K segment).  EXPECTED holds, per case, the records of the launches and clears in order -- the form, grid, block
size, dynamic LDS, and per job the rows, tile order, epilogue and (made-up) pointers, so that a cut shows as moved pointers.

EXPECTED was recorded from the launchers as they were BEFORE the planner existed (gemm.hip's plan_gemm / cut_partial_round /
split256_cut_rows and the launch functions of the five GEMM files, one printing line in front of every launch and memset, run
without a device), not from the planner: the test holds the planner to the decisions the library made before."""

CASES = []


def _g(name, head, *jobs):
    CASES.append((name, 'G %s %s ; %s' % (name, head, ' ; '.join(jobs))))


def _t(name, keys):
    CASES.append((name, 'T %s %s' % (name, keys)))


# ---- tests/test_gpu_gemm.py: every shape, under the arithmetic and tile option the test sets ----
for M, N, K in [(2048, 1024, 512), (2048, 1024, 1024), (1536, 1024, 768), (512, 2048, 512), (51712 // 8, 512, 512)]:
    for tile in (-1, 0):
        for form, keys in (('one', ''), ('splitk', 'ksplit=-1'), ('splitk2', 'ksplit=-1 kgroups=2')):
            _g('gemm_forms_%dx%dx%d_tile%d_%s' % (M, N, K, tile, form), 'tile=%d' % tile, 'M=%d N=%d K=%d %s' % (M, N, K, keys))
for M, N, K in [(51712, 512, 512), (52224, 2048, 512), (51712, 256, 512), (51712, 1024, 2048)]:
    _g('gemm_round_%dx%dx%d_one' % (M, N, K), '', 'M=%d N=%d K=%d' % (M, N, K))
    _g('gemm_round_%dx%dx%d_cut' % (M, N, K), '', 'M=%d N=%d K=%d ksplit=-1' % (M, N, K))
for M, N, K in [(8192, 2048, 768), (8192, 2048, 1024), (8192, 2048, 1536), (1024, 512, 512), (333, 200, 96)]:
    for tile in (0, 1, 2, -1):
        _g('gemm_plain_%dx%dx%d_tile%d' % (M, N, K, tile), 'tile=%d' % tile, 'M=%d N=%d K=%d' % (M, N, K))
for M in (10240, 10300, 16640, 8448, 300):
    for arith in (1, 2):
        _g('gemm_splitcut_%d_arith%d' % (M, arith), 'arith=%d' % arith, 'M=%d N=2048 K=768 bstatic=1' % M)
for K in (768, 1024, 1536):
    _g('gemm_accuracy_%d_arith0' % K, 'arith=0', 'M=8192 N=2048 K=%d' % K)
    for arith in (1, 2):
        for weight in (0, 1):
            _g('gemm_accuracy_%d_arith%d_weight%d' % (K, arith, weight), 'arith=%d' % arith, 'M=8192 N=2048 K=%d bstatic=%d' % (K, weight))
for M, N, K in [(2048, 512, 8192), (2048, 1024, 4096), (512, 512, 2048), (256, 768, 16384)]:
    for arith in (0, 2):
        _t('gemm_tn_%dx%dx%d_arith%d' % (M, N, K, arith), 'arith=%d M=%d N=%d K=%d' % (arith, M, N, K))

# ---- tests/test_gpu_split.py, the partial-round test: a search step at depth 2, width 512 (10 240 and 10 300 rows), modes 1 and 2 ----
for R, group in ((10240, 256), (10300, 100)):
    for arith in (1, 2):
        live = 'nact=%d bstatic=1' % group
        _g('search_%d_arith%d_layer1' % (R, arith), 'arith=%d epi=1' % arith,
           'M=%d N=2048 segs=128,512 rows=2 crows=1 %s' % (R, live), 'M=%d N=512 K=512 epiplain=1 %s' % (R, live))
        _g('search_%d_arith%d_top' % (R, arith), 'arith=%d epi=1' % arith, 'M=%d N=2048 segs=512,512,512 rows=4 crows=1 %s' % (R, live))
        _g('search_%d_arith%d_logits' % (R, arith), 'arith=%d epi=0' % arith, 'M=%d N=128 K=512 %s' % (R, live), 'M=%d N=512 K=512 %s' % (R, live))

# ---- a plain job with a grid of at most 128 tiles; the encoder's fused-LSTM launches at 1024 lines ----
_g('plain_small_grid', '', 'M=1024 N=1024 K=512')
_g('encoder_two_jobs_256_tiles', 'epi=1', 'M=1024 N=2048 segs=512,512 skip=2', 'M=1024 N=2048 segs=512,512 skip=2')
_g('encoder_three_jobs_384_tiles', 'epi=1', *['M=1024 N=2048 segs=512,512 skip=2'] * 3)
_g('encoder_64_rows_do_not_fill', 'epi=1', 'M=640 N=2048 segs=512,512 skip=2', 'M=640 N=2048 segs=512,512 skip=2')
_g('encoder_small_stays_32_rows', 'epi=1', 'M=512 N=2048 segs=512,512 skip=2', 'M=512 N=2048 segs=512,512 skip=2')
_g('encoder_two_jobs_ncu64', 'ncu=64 epi=1', 'M=1024 N=2048 segs=512,512 skip=2', 'M=1024 N=2048 segs=512,512 skip=2')
_g('encoder_three_jobs_ncu304', 'ncu=304 epi=1', *['M=1024 N=2048 segs=512,512 skip=2'] * 3)

# ---- train step ----
_g('train_step_data_gemm', '', 'M=512 N=2048 K=2048 ksplit=-1 kgroups=2')
_g('train_step_data_gemm_ordered', 'ordered=1', 'M=512 N=2048 K=2048 ksplit=-1 kgroups=2')
_g('train_step_data_gemm_zeroed', '', 'M=512 N=2048 K=2048 ksplit=-1 kgroups=2 zeroed=1')
_g('train_step_data_gemm_ld', '', 'M=512 N=2048 K=2048 ksplit=-1 outld=4096 slot=1048576 step=3')
_g('train_two_wave_groups', '', 'M=2048 N=1024 K=512 ksplit=-1 kgroups=2')
_g('train_round_cut', '', 'M=51712 N=512 K=512 ksplit=-1')
_g('train_round_cut_off', 'tail_cut=0', 'M=51712 N=512 K=512 ksplit=-1')
_g('train_round_three_quarters_full', '', 'M=61952 N=512 K=512 ksplit=-1')
_g('train_round_cut_64_rows', '', 'M=52224 N=2048 K=512 ksplit=-1')
_g('train_round_cut_ncu64', 'ncu=64', 'M=51712 N=512 K=512 ksplit=-1')
_g('train_round_cut_ncu64_whole_rounds_go_skinny', 'ncu=64', 'M=5120 N=512 K=256 ksplit=-1')
_g('train_round_cut_ncu304', 'ncu=304', 'M=51712 N=512 K=512 ksplit=-1')
_g('train_round_cut_gathered_rows', '', 'M=51712 N=512 K=512 ksplit=-1 rows=1')
_g('train_round_cut_under_split', 'arith=2', 'M=51712 N=512 K=512 ksplit=-1')
_g('train_cell_launch', 'epi=1', 'M=512 N=2048 K=512 zinit=1 gates=1 out2=1 kgroups=2')
_g('lds_pad', 'lds_pad=16384', 'M=8192 N=2048 K=768')

# ---- arithmetic 1 ----
_g('split1_unskinnied', 'arith=1 epi=1', 'M=1024 N=2048 segs=512,512 skip=2', 'M=1024 N=2048 segs=512,512 skip=2')
_g('split1_train_launch_stays_skinny', 'arith=1 epi=1', 'M=512 N=2048 K=512 zinit=1 gates=1 out2=1')
_g('split1_splittable_stays_skinny', 'arith=1', 'M=512 N=2048 K=2048 ksplit=-1')
_g('split1_two_wave_groups_stay_fp32', 'arith=1', 'M=2048 N=1024 K=512 ksplit=-1 kgroups=2')

# ---- arithmetic 2, N = 2048 ----
for M in (10240, 12288, 10300, 8448, 300):
    _g('split2_%d' % M, 'arith=2', 'M=%d N=2048 K=768 bstatic=1' % M)
_g('split2_12288_ncu64', 'arith=2 ncu=64', 'M=12288 N=2048 K=768 bstatic=1')
_g('split2_12288_ncu304', 'arith=2 ncu=304', 'M=12288 N=2048 K=768 bstatic=1')
_g('split2_45056_ncu304', 'arith=2 ncu=304', 'M=45056 N=2048 K=768 bstatic=1')
_g('split2_45100_ncu304', 'arith=2 ncu=304', 'M=45100 N=2048 K=768 bstatic=1')
_g('split2_nact_group_does_not_divide', 'arith=2 epi=1', 'M=10240 N=2048 segs=512,512 rows=2 crows=1 nact=768 bstatic=1')
_g('split2_nact_group_divides', 'arith=2 epi=1', 'M=10240 N=2048 segs=512,512 rows=2 crows=1 nact=256 bstatic=1')
_g('split2_four_jobs_all_cut', 'arith=2', *['M=10240 N=2048 K=768 bstatic=1'] * 4)
_g('split2_four_jobs_ragged', 'arith=2', *['M=10300 N=2048 K=768 bstatic=1'] * 4)
_g('split2_mixed', 'arith=2 epi=1', 'M=10240 N=2048 segs=512,512 rows=2 crows=1 bstatic=1', 'M=10240 N=512 K=512 epiplain=1 bstatic=1',
   'M=16384 N=2048 segs=512,512 bstatic=1', 'M=300 N=2048 segs=512,512 bstatic=1')
_g('split2_mixed_plain', 'arith=2 epi=0', 'M=16384 N=2048 K=512 bstatic=1 epiplain=1', 'M=8192 N=512 K=512 epiplain=1')
_g('split2_tail_cut_off', 'arith=2 split_tail_cut=0', 'M=10240 N=2048 K=768 bstatic=1')
_g('split2_tail_cut_off_ragged', 'arith=2 split_tail_cut=0', 'M=10300 N=2048 K=768 bstatic=1')
_g('split2_images_off', 'arith=2 images=0', 'M=8192 N=2048 K=768 bstatic=1')
_g('split2_image_of_first_job_only', 'arith=2', 'M=8192 N=2048 K=768 bstatic=1', 'M=8192 N=2048 K=768 bstatic=1 koff0=8 Ktot=784')
_g('split2_no_cell_state', 'arith=2 epi=1', 'M=8192 N=2048 segs=512,512 cell=0 bstatic=1')
_g('split2_accumulate', 'arith=2', 'M=8192 N=2048 K=768 acc=1')
_g('split2_first_state', 'arith=2 epi=1', 'M=10240 N=2048 segs=512,512 first=2 bstatic=1')
for tile in (0, 1, 2):
    _g('split2_tile%d' % tile, 'arith=2 tile=%d' % tile, 'M=10240 N=2048 K=768 bstatic=1')
    _g('encoder_tile%d' % tile, 'epi=1 tile=%d' % tile, 'M=1024 N=2048 segs=512,512 skip=2', 'M=1024 N=2048 segs=512,512 skip=2')

# ---- weight gradients ----
TN_SHAPES = {
    'split_form': 'M=2048 N=2048 K=51712',
    'short_k': 'M=2048 N=2048 K=1008',
    'padded_rows': 'M=768 Mstore=640 N=2048 K=51712',
    'too_few_tiles': 'M=256 N=256 K=2048',
    'one_share': 'M=4096 N=4096 K=4096',
    'fp32_only_shape': 'M=640 N=2048 K=51712',
    'row_stride': 'M=2048 N=512 K=8192 ldc=640',
}
for shape, keys in TN_SHAPES.items():
    for arith in (0, 2):
        _t('tn_%s_arith%d' % (shape, arith), 'arith=%d %s' % (arith, keys))
        _t('tn_%s_arith%d_ordered' % (shape, arith), 'arith=%d ordered_ws=1 %s' % (arith, keys))
    _t('tn_%s_accumulate' % shape, 'arith=2 acc=1 %s' % keys)
    _t('tn_%s_zeroed' % shape, 'arith=2 zeroed=1 %s' % keys)
    _t('tn_%s_split_off' % shape, 'arith=2 tn_split=0 %s' % keys)
    _t('tn_%s_split_off_ordered' % shape, 'arith=2 tn_split=0 ordered_ws=1 %s' % keys)
    for ncu in (64, 304):
        _t('tn_%s_ncu%d' % (shape, ncu), 'arith=2 ncu=%d %s' % (ncu, keys))
        _t('tn_%s_ncu%d_ordered' % (shape, ncu), 'arith=2 ncu=%d ordered_ws=1 %s' % (ncu, keys))

EXPECTED = {
    'gemm_forms_2048x1024x512_tile-1_one': [
        'L k32 epi=0 grid=512,1,1 block=256 lds=0 img=0/0 | M=2048 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x512_tile-1_splitk': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128 epi=0 grid=128,1,2 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x512_tile-1_splitk2': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128x2 epi=0 grid=128,1,2 block=512 lds=110592 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x512_tile0_one': [
        'L g128 epi=0 grid=128,1,1 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x512_tile0_splitk': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128 epi=0 grid=128,1,2 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x512_tile0_splitk2': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128x2 epi=0 grid=128,1,2 block=512 lds=110592 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x1024_tile-1_one': [
        'L k32 epi=0 grid=512,1,1 block=256 lds=0 img=0/0 | M=2048 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x1024_tile-1_splitk': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128 epi=0 grid=128,1,4 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x1024_tile-1_splitk2': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128 epi=0 grid=128,1,4 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x1024_tile0_one': [
        'L g128 epi=0 grid=128,1,1 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x1024_tile0_splitk': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128 epi=0 grid=128,1,4 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_2048x1024x1024_tile0_splitk2': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128 epi=0 grid=128,1,4 block=256 lds=69632 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_1536x1024x768_tile-1_one': [
        'L k32 epi=0 grid=384,1,1 block=256 lds=0 img=0/0 | M=1536 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_1536x1024x768_tile-1_splitk': [
        'C 11000000000 rows=1536 cols=1024 ld=1024',
        'L k32 epi=0 grid=384,1,3 block=256 lds=0 img=0/0 | M=1536 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_1536x1024x768_tile-1_splitk2': [
        'C 11000000000 rows=1536 cols=1024 ld=1024',
        'L k32 epi=0 grid=384,1,3 block=256 lds=0 img=0/0 | M=1536 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_1536x1024x768_tile0_one': [
        'L g128 epi=0 grid=96,1,1 block=256 lds=69632 img=0/0 | M=1536 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_1536x1024x768_tile0_splitk': [
        'C 11000000000 rows=1536 cols=1024 ld=1024',
        'L g128 epi=0 grid=96,1,3 block=256 lds=69632 img=0/0 | M=1536 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_1536x1024x768_tile0_splitk2': [
        'C 11000000000 rows=1536 cols=1024 ld=1024',
        'L g128 epi=0 grid=96,1,3 block=256 lds=69632 img=0/0 | M=1536 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_512x2048x512_tile-1_one': [
        'L k32 epi=0 grid=256,1,1 block=256 lds=0 img=0/0 | M=512 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_512x2048x512_tile-1_splitk': [
        'C 11000000000 rows=512 cols=2048 ld=2048',
        'L k32 epi=0 grid=256,1,2 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_512x2048x512_tile-1_splitk2': [
        'C 11000000000 rows=512 cols=2048 ld=2048',
        'L k32 epi=0 grid=256,1,2 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_512x2048x512_tile0_one': [
        'L g128 epi=0 grid=64,1,1 block=256 lds=69632 img=0/0 | M=512 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_512x2048x512_tile0_splitk': [
        'C 11000000000 rows=512 cols=2048 ld=2048',
        'L g128 epi=0 grid=64,1,2 block=256 lds=69632 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_512x2048x512_tile0_splitk2': [
        'C 11000000000 rows=512 cols=2048 ld=2048',
        'L g128x2 epi=0 grid=64,1,2 block=512 lds=110592 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_6464x512x512_tile-1_one': [
        'L g128 epi=0 grid=204,1,1 block=256 lds=69632 img=0/0 | M=6464 N=512 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_6464x512x512_tile-1_splitk': [
        'C 11000000000 rows=6464 cols=512 ld=512',
        'L k32 epi=0 grid=808,1,2 block=256 lds=0 img=0/0 | M=6464 N=512 ks=-1 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_6464x512x512_tile-1_splitk2': [
        'C 11000000000 rows=6464 cols=512 ld=512',
        'L k32 epi=0 grid=808,1,2 block=256 lds=0 img=0/0 | M=6464 N=512 ks=-1 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_6464x512x512_tile0_one': [
        'L g128 epi=0 grid=204,1,1 block=256 lds=69632 img=0/0 | M=6464 N=512 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_6464x512x512_tile0_splitk': [
        'C 11000000000 rows=6464 cols=512 ld=512',
        'L g128 epi=0 grid=204,1,2 block=256 lds=69632 img=0/0 | M=6464 N=512 ks=-1 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_forms_6464x512x512_tile0_splitk2': [
        'C 11000000000 rows=6464 cols=512 ld=512',
        'L g128 epi=0 grid=204,1,2 block=256 lds=69632 img=0/0 | M=6464 N=512 ks=-1 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_51712x512x512_one': [
        'L g128 epi=0 grid=1616,1,1 block=256 lds=69632 img=0/0 | M=51712 N=512 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_51712x512x512_cut': [
        'L g128 epi=0 grid=1536,1,1 block=256 lds=69632 img=0/0 | M=49152 N=512 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k32 epi=0 grid=320,1,1 block=256 lds=0 img=0/0 | M=2560 N=512 ks=0 xcd=0 ep=0 a0=10106000000/0/0 c=0/0/0 o=11006000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_52224x2048x512_one': [
        'L g128 epi=0 grid=6528,1,1 block=256 lds=69632 img=0/0 | M=52224 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_52224x2048x512_cut': [
        'L g128 epi=0 grid=6144,1,1 block=256 lds=69632 img=0/0 | M=49152 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k64 epi=0 grid=768,1,1 block=256 lds=0 img=0/0 | M=3072 N=2048 ks=0 xcd=0 ep=0 a0=10106000000/0/0 c=0/0/0 o=11018000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_51712x256x512_one': [
        'L g128 epi=0 grid=808,1,1 block=256 lds=69632 img=0/0 | M=51712 N=256 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_51712x256x512_cut': [
        'L g128 epi=0 grid=512,1,1 block=256 lds=69632 img=0/0 | M=32768 N=256 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k64 epi=0 grid=592,1,1 block=256 lds=0 img=0/0 | M=18944 N=256 ks=0 xcd=0 ep=0 a0=10104000000/0/0 c=0/0/0 o=11002000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_51712x1024x2048_one': [
        'L g128 epi=0 grid=3232,1,1 block=256 lds=69632 img=0/0 | M=51712 N=1024 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_round_51712x1024x2048_cut': [
        'L g128 epi=0 grid=3072,1,1 block=256 lds=69632 img=0/0 | M=49152 N=1024 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k32 epi=0 grid=640,1,1 block=256 lds=0 img=0/0 | M=2560 N=1024 ks=0 xcd=0 ep=0 a0=10118000000/0/0 c=0/0/0 o=1100c000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x768_tile0': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x768_tile1': [
        'L k32 epi=0 grid=4096,1,1 block=256 lds=0 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x768_tile2': [
        'L k64 epi=0 grid=2048,1,1 block=256 lds=0 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x768_tile-1': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1024_tile0': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1024_tile1': [
        'L k32 epi=0 grid=4096,1,1 block=256 lds=0 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1024_tile2': [
        'L k64 epi=0 grid=2048,1,1 block=256 lds=0 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1024_tile-1': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1536_tile0': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1536_tile1': [
        'L k32 epi=0 grid=4096,1,1 block=256 lds=0 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1536_tile2': [
        'L k64 epi=0 grid=2048,1,1 block=256 lds=0 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_8192x2048x1536_tile-1': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_1024x512x512_tile0': [
        'L g128 epi=0 grid=32,1,1 block=256 lds=69632 img=0/0 | M=1024 N=512 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_1024x512x512_tile1': [
        'L k32 epi=0 grid=128,1,1 block=256 lds=0 img=0/0 | M=1024 N=512 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_1024x512x512_tile2': [
        'L k64 epi=0 grid=64,1,1 block=256 lds=0 img=0/0 | M=1024 N=512 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_1024x512x512_tile-1': [
        'L k32 epi=0 grid=128,1,1 block=256 lds=0 img=0/0 | M=1024 N=512 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_333x200x96_tile0': [
        'L g128 epi=0 grid=6,1,1 block=256 lds=69632 img=0/0 | M=333 N=200 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_333x200x96_tile1': [
        'L k32 epi=0 grid=22,1,1 block=256 lds=0 img=0/0 | M=333 N=200 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_333x200x96_tile2': [
        'L k64 epi=0 grid=12,1,1 block=256 lds=0 img=0/0 | M=333 N=200 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_plain_333x200x96_tile-1': [
        'L k32 epi=0 grid=22,1,1 block=256 lds=0 img=0/0 | M=333 N=200 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_10240_arith1': [
        'L s128 epi=0 grid=1280,1,1 block=256 lds=77824 img=0/0 | M=10240 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_10240_arith2': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_10300_arith1': [
        'L s128 epi=0 grid=1296,1,1 block=256 lds=77824 img=0/0 | M=10300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_10300_arith2': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=272,1,1 block=256 lds=77824 img=0/0 | M=2108 N=2048 ks=0 xcd=1 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_16640_arith1': [
        'L s128 epi=0 grid=2080,1,1 block=256 lds=77824 img=0/0 | M=16640 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_16640_arith2': [
        'L s256 epi=0 grid=512,1,1 block=512 lds=163840 img=1/1 | M=16384 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10103000000/0/0 c=0/0/0 o=11008000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_8448_arith1': [
        'L s128 epi=0 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_8448_arith2': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_300_arith1': [
        'L s128 epi=0 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_splitcut_300_arith2': [
        'L s128 epi=0 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_768_arith0': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_768_arith1_weight0': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_768_arith1_weight1': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_768_arith2_weight0': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_768_arith2_weight1': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1024_arith0': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1024_arith1_weight0': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1024_arith1_weight1': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1024_arith2_weight0': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1024_arith2_weight1': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1536_arith0': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=69632 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1536_arith1_weight0': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1536_arith1_weight1': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1536_arith2_weight0': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_accuracy_1536_arith2_weight1': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'gemm_tn_2048x512x8192_arith0': [
        'C 10300000000 rows=2048 cols=512 ld=512',
        'T tn grid=512 block=256 lds=0 nsplit=8 part=0 colpart=0',
        '=> split=0 shares=8 nonempty=8 floats=8404992',
    ],
    'gemm_tn_2048x512x8192_arith2': [
        'C 10300000000 rows=2048 cols=512 ld=512',
        'T tns grid=128 block=512 lds=98304 nsplit=8 part=0 colpart=0',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
    'gemm_tn_2048x1024x4096_arith0': [
        'C 10300000000 rows=2048 cols=1024 ld=1024',
        'T tn grid=512 block=256 lds=0 nsplit=4 part=0 colpart=0',
        '=> split=0 shares=4 nonempty=4 floats=8396800',
    ],
    'gemm_tn_2048x1024x4096_arith2': [
        'C 10300000000 rows=2048 cols=1024 ld=1024',
        'T tns grid=128 block=512 lds=98304 nsplit=4 part=0 colpart=0',
        '=> split=1 shares=4 nonempty=4 floats=8396800',
    ],
    'gemm_tn_512x512x2048_arith0': [
        'C 10300000000 rows=512 cols=512 ld=512',
        'T tn grid=32 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=525312',
    ],
    'gemm_tn_512x512x2048_arith2': [
        'C 10300000000 rows=512 cols=512 ld=512',
        'T tn grid=32 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=525312',
    ],
    'gemm_tn_256x768x16384_arith0': [
        'C 10300000000 rows=256 cols=768 ld=768',
        'T tn grid=192 block=256 lds=0 nsplit=16 part=0 colpart=0',
        '=> split=0 shares=16 nonempty=16 floats=3149824',
    ],
    'gemm_tn_256x768x16384_arith2': [
        'C 10300000000 rows=256 cols=768 ld=768',
        'T tn grid=192 block=256 lds=0 nsplit=16 part=0 colpart=0',
        '=> split=0 shares=16 nonempty=16 floats=3149824',
    ],
    'search_10240_arith1_layer1': [
        'L s128 epi=1 grid=1280,2,1 block=256 lds=77824 img=0/0 | M=10240 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000 | M=10240 N=512 ks=0 xcd=0 ep=1 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10240_arith1_top': [
        'L s128 epi=1 grid=1280,1,1 block=256 lds=77824 img=0/0 | M=10240 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 a2=10300000000/10a00000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'search_10240_arith1_logits': [
        'L s128 epi=0 grid=320,2,1 block=256 lds=77824 img=0/0 | M=10240 N=128 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=11500000000 | M=10240 N=512 ks=0 xcd=8 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10240_arith2_layer1': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=320,2,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=0 ep=0 a0=10100400000/0/0 a1=10200000000/10900008000/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500000080 | M=10240 N=512 ks=0 xcd=8 ep=1 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10240_arith2_top': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 a2=10300000000/10a00000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101000000/0/0 a1=10201000000/0/0 a2=10300000000/10a00008000/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500000080',
    ],
    'search_10240_arith2_logits': [
        'L s128 epi=0 grid=320,2,1 block=256 lds=77824 img=0/0 | M=10240 N=128 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=11500000000 | M=10240 N=512 ks=0 xcd=8 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10300_arith1_layer1': [
        'L s128 epi=1 grid=1296,2,1 block=256 lds=77824 img=0/0 | M=10300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000 | M=10300 N=512 ks=0 xcd=0 ep=1 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10300_arith1_top': [
        'L s128 epi=1 grid=1296,1,1 block=256 lds=77824 img=0/0 | M=10300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 a2=10300000000/10a00000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'search_10300_arith1_logits': [
        'L s128 epi=0 grid=324,2,1 block=256 lds=77824 img=0/0 | M=10300 N=128 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=11500000000 | M=10300 N=512 ks=0 xcd=0 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10300_arith2_layer1': [
        'L s128 epi=1 grid=1296,2,1 block=256 lds=77824 img=0/0 | M=10300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000 | M=10300 N=512 ks=0 xcd=0 ep=1 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'search_10300_arith2_top': [
        'L s128 epi=1 grid=1296,1,1 block=256 lds=77824 img=0/0 | M=10300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 a2=10300000000/10a00000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'search_10300_arith2_logits': [
        'L s128 epi=0 grid=324,2,1 block=256 lds=77824 img=0/0 | M=10300 N=128 ks=0 xcd=0 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=11500000000 | M=10300 N=512 ks=0 xcd=0 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=21500000000',
    ],
    'plain_small_grid': [
        'L k32 epi=0 grid=256,1,1 block=256 lds=0 img=0/0 | M=1024 N=1024 ks=0 xcd=2 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'encoder_two_jobs_256_tiles': [
        'L k64 epi=1 grid=256,2,1 block=256 lds=0 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'encoder_three_jobs_384_tiles': [
        'L k64 epi=1 grid=256,3,1 block=256 lds=0 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=30100000000/0/0 a1=30200000000/0/0 c=30400000000/0/0 o=31000000000 co=31100000000 z=0 go=0 o2=0 na=0',
    ],
    'encoder_64_rows_do_not_fill': [
        'L g128 epi=1 grid=80,2,1 block=256 lds=69632 img=0/0 | M=640 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=640 N=2048 ks=0 xcd=1 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'encoder_small_stays_32_rows': [
        'L k32 epi=1 grid=256,2,1 block=256 lds=0 img=0/0 | M=512 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=512 N=2048 ks=0 xcd=1 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'encoder_two_jobs_ncu64': [
        'L g128 epi=1 grid=128,2,1 block=256 lds=69632 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'encoder_three_jobs_ncu304': [
        'L k64 epi=1 grid=256,3,1 block=256 lds=0 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=30100000000/0/0 a1=30200000000/0/0 c=30400000000/0/0 o=31000000000 co=31100000000 z=0 go=0 o2=0 na=0',
    ],
    'train_step_data_gemm': [
        'C 11000000000 rows=512 cols=2048 ld=2048',
        'L k32 epi=0 grid=256,1,2 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_step_data_gemm_ordered': [
        'L k32 epi=0 grid=256,1,1 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_step_data_gemm_zeroed': [
        'L k32 epi=0 grid=256,1,2 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_step_data_gemm_ld': [
        'C 11000c00000 rows=512 cols=2048 ld=4096',
        'L k32 epi=0 grid=256,1,2 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_two_wave_groups': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128x2 epi=0 grid=128,1,2 block=512 lds=110592 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut': [
        'L g128 epi=0 grid=1536,1,1 block=256 lds=69632 img=0/0 | M=49152 N=512 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k32 epi=0 grid=320,1,1 block=256 lds=0 img=0/0 | M=2560 N=512 ks=0 xcd=0 ep=0 a0=10106000000/0/0 c=0/0/0 o=11006000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_off': [
        'L g128 epi=0 grid=1616,1,1 block=256 lds=69632 img=0/0 | M=51712 N=512 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_three_quarters_full': [
        'L g128 epi=0 grid=1936,1,1 block=256 lds=69632 img=0/0 | M=61952 N=512 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_64_rows': [
        'L g128 epi=0 grid=6144,1,1 block=256 lds=69632 img=0/0 | M=49152 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k64 epi=0 grid=768,1,1 block=256 lds=0 img=0/0 | M=3072 N=2048 ks=0 xcd=0 ep=0 a0=10106000000/0/0 c=0/0/0 o=11018000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_ncu64': [
        'L g128 epi=0 grid=1536,1,1 block=256 lds=69632 img=0/0 | M=49152 N=512 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k64 epi=0 grid=160,1,1 block=256 lds=0 img=0/0 | M=2560 N=512 ks=0 xcd=0 ep=0 a0=10106000000/0/0 c=0/0/0 o=11006000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_ncu64_whole_rounds_go_skinny': [
        'L k32 epi=0 grid=512,1,1 block=256 lds=0 img=0/0 | M=4096 N=512 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k32 epi=0 grid=128,1,1 block=256 lds=0 img=0/0 | M=1024 N=512 ks=0 xcd=0 ep=0 a0=10100400000/0/0 c=0/0/0 o=11000800000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_ncu304': [
        'L g128 epi=0 grid=1216,1,1 block=256 lds=69632 img=0/0 | M=38912 N=512 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L k64 epi=0 grid=800,1,1 block=256 lds=0 img=0/0 | M=12800 N=512 ks=0 xcd=0 ep=0 a0=10104c00000/0/0 c=0/0/0 o=11004c00000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_gathered_rows': [
        'L g128 epi=0 grid=1616,1,1 block=256 lds=69632 img=0/0 | M=51712 N=512 ks=-1 xcd=4 ep=0 a0=10100000000/10800000000/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_round_cut_under_split': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=0/0 | M=32768 N=512 ks=-1 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s256 epi=0 grid=148,1,1 block=512 lds=163840 img=0/0 | M=18944 N=512 ks=-1 xcd=0 ep=0 a0=10104000000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'train_cell_launch': [
        'L k32 epi=1 grid=256,1,1 block=256 lds=0 img=0/0 | M=512 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
    'lds_pad': [
        'L g128 epi=0 grid=1024,1,1 block=256 lds=86016 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split1_unskinnied': [
        'L s128 epi=1 grid=128,2,1 block=256 lds=77824 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'split1_train_launch_stays_skinny': [
        'L k32 epi=1 grid=256,1,1 block=256 lds=0 img=0/0 | M=512 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
    'split1_splittable_stays_skinny': [
        'C 11000000000 rows=512 cols=2048 ld=2048',
        'L k32 epi=0 grid=256,1,2 block=256 lds=0 img=0/0 | M=512 N=2048 ks=-1 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split1_two_wave_groups_stay_fp32': [
        'C 11000000000 rows=2048 cols=1024 ld=1024',
        'L g128x2 epi=0 grid=128,1,2 block=512 lds=110592 img=0/0 | M=2048 N=1024 ks=-1 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_10240': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_12288': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s256 epi=0 grid=128,1,1 block=512 lds=163840 img=1/1 | M=4096 N=2048 ks=0 xcd=4 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_10300': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=272,1,1 block=256 lds=77824 img=0/0 | M=2108 N=2048 ks=0 xcd=1 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_8448': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_300': [
        'L s128 epi=0 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_12288_ncu64': [
        'L s256 epi=0 grid=384,1,1 block=512 lds=163840 img=1/1 | M=12288 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_12288_ncu304': [
        'L s256 epi=0 grid=304,1,1 block=512 lds=163840 img=1/1 | M=9728 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=320,1,1 block=256 lds=77824 img=0/0 | M=2560 N=2048 ks=0 xcd=4 ep=0 a0=10101c80000/0/0 c=0/0/0 o=11004c00000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_45056_ncu304': [
        'L s256 epi=0 grid=1216,1,1 block=512 lds=163840 img=1/1 | M=38912 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s256 epi=0 grid=192,1,1 block=512 lds=163840 img=1/1 | M=6144 N=2048 ks=0 xcd=4 ep=0 a0=10107200000/0/0 c=0/0/0 o=11013000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_45100_ncu304': [
        'L s256 epi=0 grid=1216,1,1 block=512 lds=163840 img=1/1 | M=38912 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s256 epi=0 grid=192,1,1 block=512 lds=163840 img=1/1 | M=6144 N=2048 ks=0 xcd=4 ep=0 a0=10107200000/0/0 c=0/0/0 o=11013000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=16,1,1 block=256 lds=77824 img=0/0 | M=44 N=2048 ks=0 xcd=1 ep=0 a0=10108400000/0/0 c=0/0/0 o=11016000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_nact_group_does_not_divide': [
        'L s256 epi=1 grid=320,1,1 block=512 lds=163840 img=1/1 | M=10240 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'split2_nact_group_divides': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101000000/0/0 a1=10200000000/10900008000/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500000080',
    ],
    'split2_four_jobs_all_cut': [
        'L s256 epi=0 grid=256,4,1 block=512 lds=163840 img=1/4 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=30100000000/0/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=40100000000/0/0 c=0/0/0 o=41000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,4,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=20101800000/0/0 c=0/0/0 o=21004000000 co=0 z=0 go=0 o2=0 na=0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=30101800000/0/0 c=0/0/0 o=31004000000 co=0 z=0 go=0 o2=0 na=0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=40101800000/0/0 c=0/0/0 o=41004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_four_jobs_ragged': [
        'L s256 epi=0 grid=256,4,1 block=512 lds=163840 img=1/4 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=30100000000/0/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=40100000000/0/0 c=0/0/0 o=41000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=272,4,1 block=256 lds=77824 img=0/0 | M=2108 N=2048 ks=0 xcd=1 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0 | M=2108 N=2048 ks=0 xcd=1 ep=0 a0=20101800000/0/0 c=0/0/0 o=21004000000 co=0 z=0 go=0 o2=0 na=0 | M=2108 N=2048 ks=0 xcd=1 ep=0 a0=30101800000/0/0 c=0/0/0 o=31004000000 co=0 z=0 go=0 o2=0 na=0 | M=2108 N=2048 ks=0 xcd=1 ep=0 a0=40101800000/0/0 c=0/0/0 o=41004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_mixed': [
        'L s256 epi=1 grid=512,2,1 block=512 lds=163840 img=1/2 | M=8192 N=2048 ks=0 xcd=0 ep=0 a0=10100000000/0/0 a1=10200000000/10900000000/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=16384 N=2048 ks=0 xcd=8 ep=0 a0=30100000000/0/0 a1=30200000000/0/0 c=30400000000/0/0 o=31000000000 co=31100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=320,3,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=0 ep=0 a0=10101000000/0/0 a1=10200000000/10900008000/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0 | M=10240 N=512 ks=0 xcd=8 ep=1 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0 | M=300 N=2048 ks=0 xcd=0 ep=0 a0=40100000000/0/0 a1=40200000000/0/0 c=40400000000/0/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'split2_mixed_plain': [
        'L s256 epi=0 grid=512,1,1 block=512 lds=163840 img=1/1 | M=16384 N=2048 ks=0 xcd=8 ep=1 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,1,1 block=256 lds=77824 img=0/0 | M=8192 N=512 ks=0 xcd=8 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_tail_cut_off': [
        'L s256 epi=0 grid=320,1,1 block=512 lds=163840 img=1/1 | M=10240 N=2048 ks=0 xcd=8 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_tail_cut_off_ragged': [
        'L s128 epi=0 grid=1296,1,1 block=256 lds=77824 img=0/0 | M=10300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_images_off': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_image_of_first_job_only': [
        'L s256 epi=0 grid=256,2,1 block=512 lds=163840 img=0/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=20100000000/0/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_no_cell_state': [
        'L s128 epi=1 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_accumulate': [
        'L s128 epi=0 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'split2_first_state': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 a1=10200000000/0/10d00000000 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101000000/0/0 a1=10201000000/0/10d01000000 c=10401000000/0/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'split2_tile0': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'encoder_tile0': [
        'L g128 epi=1 grid=128,2,1 block=256 lds=69632 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'split2_tile1': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'encoder_tile1': [
        'L k32 epi=1 grid=512,2,1 block=256 lds=0 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'split2_tile2': [
        'L s256 epi=0 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=0 grid=256,1,1 block=256 lds=77824 img=0/0 | M=2048 N=2048 ks=0 xcd=2 ep=0 a0=10101800000/0/0 c=0/0/0 o=11004000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'encoder_tile2': [
        'L k64 epi=1 grid=256,2,1 block=256 lds=0 img=0/0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/0/0 a1=10200000000/0/0 c=10400000000/0/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=1024 N=2048 ks=0 xcd=2 ep=0 a0=20100000000/0/0 a1=20200000000/0/0 c=20400000000/0/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'tn_split_form_arith0': [
        'C 10300000000 rows=2048 cols=2048 ld=2048',
        'T tn grid=512 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=8392704',
    ],
    'tn_split_form_arith0_ordered': [
        'T tn_part grid=512 block=256 lds=0 nsplit=2 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=8392704',
    ],
    'tn_split_form_arith2': [
        'C 10300000000 rows=2048 cols=2048 ld=2048',
        'T tns grid=256 block=512 lds=98304 nsplit=4 part=0 colpart=0',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_split_form_arith2_ordered': [
        'T tns_part grid=256 block=512 lds=98304 nsplit=4 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=4',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_split_form_accumulate': [
        'T tns grid=256 block=512 lds=98304 nsplit=4 part=0 colpart=0',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_split_form_zeroed': [
        'T tns grid=256 block=512 lds=98304 nsplit=4 part=0 colpart=0',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_split_form_split_off': [
        'C 10300000000 rows=2048 cols=2048 ld=2048',
        'T tn grid=512 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=8392704',
    ],
    'tn_split_form_split_off_ordered': [
        'T tn_part grid=512 block=256 lds=0 nsplit=2 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=8392704',
    ],
    'tn_split_form_ncu64': [
        'T tns grid=64 block=512 lds=98304 nsplit=1 part=0 colpart=0',
        '=> split=1 shares=1 nonempty=1 floats=16785408',
    ],
    'tn_split_form_ncu64_ordered': [
        'T tns_part grid=256 block=512 lds=98304 nsplit=4 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=4',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_split_form_ncu304': [
        'C 10300000000 rows=2048 cols=2048 ld=2048',
        'T tns grid=256 block=512 lds=98304 nsplit=4 part=0 colpart=0',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_split_form_ncu304_ordered': [
        'T tns_part grid=256 block=512 lds=98304 nsplit=4 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=4',
        '=> split=1 shares=4 nonempty=4 floats=16785408',
    ],
    'tn_short_k_arith0': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_arith0_ordered': [
        'T tn_part grid=256 block=256 lds=0 nsplit=1 part=10400000000 colpart=10401000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_arith2': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_arith2_ordered': [
        'T tn_part grid=256 block=256 lds=0 nsplit=1 part=10400000000 colpart=10401000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_accumulate': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_zeroed': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_split_off': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_split_off_ordered': [
        'T tn_part grid=256 block=256 lds=0 nsplit=1 part=10400000000 colpart=10401000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_ncu64': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_ncu64_ordered': [
        'T tn_part grid=256 block=256 lds=0 nsplit=1 part=10400000000 colpart=10401000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_ncu304': [
        'T tn grid=256 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_short_k_ncu304_ordered': [
        'T tn_part grid=256 block=256 lds=0 nsplit=1 part=10400000000 colpart=10401000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=4196352',
    ],
    'tn_padded_rows_arith0': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=576 block=256 lds=0 nsplit=6 part=0 colpart=0',
        '=> split=0 shares=6 nonempty=6 floats=7868160',
    ],
    'tn_padded_rows_arith0_ordered': [
        'T tn_part grid=576 block=256 lds=0 nsplit=6 part=10400000000 colpart=10401e00000',
        'R grid=2048 nz=6',
        '=> split=0 shares=6 nonempty=6 floats=7868160',
    ],
    'tn_padded_rows_arith2': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tns grid=240 block=512 lds=98304 nsplit=10 part=0 colpart=0',
        '=> split=1 shares=10 nonempty=10 floats=13113600',
    ],
    'tn_padded_rows_arith2_ordered': [
        'T tns_part grid=240 block=512 lds=98304 nsplit=10 part=10400000000 colpart=10403200000',
        'R grid=2048 nz=10',
        '=> split=1 shares=10 nonempty=10 floats=13113600',
    ],
    'tn_padded_rows_accumulate': [
        'T tns grid=240 block=512 lds=98304 nsplit=10 part=0 colpart=0',
        '=> split=1 shares=10 nonempty=10 floats=13113600',
    ],
    'tn_padded_rows_zeroed': [
        'T tns grid=240 block=512 lds=98304 nsplit=10 part=0 colpart=0',
        '=> split=1 shares=10 nonempty=10 floats=13113600',
    ],
    'tn_padded_rows_split_off': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=576 block=256 lds=0 nsplit=6 part=0 colpart=0',
        '=> split=0 shares=6 nonempty=6 floats=7868160',
    ],
    'tn_padded_rows_split_off_ordered': [
        'T tn_part grid=576 block=256 lds=0 nsplit=6 part=10400000000 colpart=10401e00000',
        'R grid=2048 nz=6',
        '=> split=0 shares=6 nonempty=6 floats=7868160',
    ],
    'tn_padded_rows_ncu64': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tns grid=48 block=512 lds=98304 nsplit=2 part=0 colpart=0',
        '=> split=1 shares=2 nonempty=2 floats=13113600',
    ],
    'tn_padded_rows_ncu64_ordered': [
        'T tns_part grid=240 block=512 lds=98304 nsplit=10 part=10400000000 colpart=10403200000',
        'R grid=2048 nz=10',
        '=> split=1 shares=10 nonempty=10 floats=13113600',
    ],
    'tn_padded_rows_ncu304': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tns grid=288 block=512 lds=98304 nsplit=12 part=0 colpart=0',
        '=> split=1 shares=12 nonempty=12 floats=13113600',
    ],
    'tn_padded_rows_ncu304_ordered': [
        'T tns_part grid=240 block=512 lds=98304 nsplit=10 part=10400000000 colpart=10403200000',
        'R grid=2048 nz=10',
        '=> split=1 shares=10 nonempty=10 floats=13113600',
    ],
    'tn_too_few_tiles_arith0': [
        'C 10300000000 rows=256 cols=256 ld=256',
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_arith0_ordered': [
        'T tn_part grid=8 block=256 lds=0 nsplit=2 part=10400000000 colpart=10400080000',
        'R grid=256 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_arith2': [
        'C 10300000000 rows=256 cols=256 ld=256',
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_arith2_ordered': [
        'T tn_part grid=8 block=256 lds=0 nsplit=2 part=10400000000 colpart=10400080000',
        'R grid=256 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_accumulate': [
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_zeroed': [
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_split_off': [
        'C 10300000000 rows=256 cols=256 ld=256',
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_split_off_ordered': [
        'T tn_part grid=8 block=256 lds=0 nsplit=2 part=10400000000 colpart=10400080000',
        'R grid=256 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_ncu64': [
        'C 10300000000 rows=256 cols=256 ld=256',
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_ncu64_ordered': [
        'T tn_part grid=8 block=256 lds=0 nsplit=2 part=10400000000 colpart=10400080000',
        'R grid=256 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_ncu304': [
        'C 10300000000 rows=256 cols=256 ld=256',
        'T tn grid=8 block=256 lds=0 nsplit=2 part=0 colpart=0',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_too_few_tiles_ncu304_ordered': [
        'T tn_part grid=8 block=256 lds=0 nsplit=2 part=10400000000 colpart=10400080000',
        'R grid=256 nz=2',
        '=> split=0 shares=2 nonempty=2 floats=131584',
    ],
    'tn_one_share_arith0': [
        'T tn grid=1024 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_arith0_ordered': [
        'T tn_part grid=1024 block=256 lds=0 nsplit=1 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_arith2': [
        'T tns grid=256 block=512 lds=98304 nsplit=1 part=0 colpart=0',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_arith2_ordered': [
        'T tns_part grid=256 block=512 lds=98304 nsplit=1 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=1',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_accumulate': [
        'T tns grid=256 block=512 lds=98304 nsplit=1 part=0 colpart=0',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_zeroed': [
        'T tns grid=256 block=512 lds=98304 nsplit=1 part=0 colpart=0',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_split_off': [
        'T tn grid=1024 block=256 lds=0 nsplit=1 part=0 colpart=0',
        '=> split=0 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_split_off_ordered': [
        'T tn_part grid=1024 block=256 lds=0 nsplit=1 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=1',
        '=> split=0 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_ncu64': [
        'T tns grid=256 block=512 lds=98304 nsplit=1 part=0 colpart=0',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_ncu64_ordered': [
        'T tns_part grid=256 block=512 lds=98304 nsplit=1 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=1',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_ncu304': [
        'T tns grid=256 block=512 lds=98304 nsplit=1 part=0 colpart=0',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_one_share_ncu304_ordered': [
        'T tns_part grid=256 block=512 lds=98304 nsplit=1 part=10400000000 colpart=10404000000',
        'R grid=2048 nz=1',
        '=> split=1 shares=1 nonempty=1 floats=16781312',
    ],
    'tn_fp32_only_shape_arith0': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_arith0_ordered': [
        'T tn_part grid=560 block=256 lds=0 nsplit=7 part=10400000000 colpart=10402300000',
        'R grid=2048 nz=7',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_arith2': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_arith2_ordered': [
        'T tn_part grid=560 block=256 lds=0 nsplit=7 part=10400000000 colpart=10402300000',
        'R grid=2048 nz=7',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_accumulate': [
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_zeroed': [
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_split_off': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_split_off_ordered': [
        'T tn_part grid=560 block=256 lds=0 nsplit=7 part=10400000000 colpart=10402300000',
        'R grid=2048 nz=7',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_ncu64': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_ncu64_ordered': [
        'T tn_part grid=560 block=256 lds=0 nsplit=7 part=10400000000 colpart=10402300000',
        'R grid=2048 nz=7',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_ncu304': [
        'C 10300000000 rows=640 cols=2048 ld=2048',
        'T tn grid=560 block=256 lds=0 nsplit=7 part=0 colpart=0',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_fp32_only_shape_ncu304_ordered': [
        'T tn_part grid=560 block=256 lds=0 nsplit=7 part=10400000000 colpart=10402300000',
        'R grid=2048 nz=7',
        '=> split=0 shares=7 nonempty=7 floats=9179520',
    ],
    'tn_row_stride_arith0': [
        'C 10300000000 rows=2048 cols=512 ld=640',
        'T tn grid=512 block=256 lds=0 nsplit=8 part=0 colpart=0',
        '=> split=0 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_arith0_ordered': [
        'T tn_part grid=512 block=256 lds=0 nsplit=8 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=8',
        '=> split=0 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_arith2': [
        'C 10300000000 rows=2048 cols=512 ld=640',
        'T tns grid=128 block=512 lds=98304 nsplit=8 part=0 colpart=0',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_arith2_ordered': [
        'T tns_part grid=128 block=512 lds=98304 nsplit=8 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=8',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_accumulate': [
        'T tns grid=128 block=512 lds=98304 nsplit=8 part=0 colpart=0',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_zeroed': [
        'T tns grid=128 block=512 lds=98304 nsplit=8 part=0 colpart=0',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_split_off': [
        'C 10300000000 rows=2048 cols=512 ld=640',
        'T tn grid=512 block=256 lds=0 nsplit=8 part=0 colpart=0',
        '=> split=0 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_split_off_ordered': [
        'T tn_part grid=512 block=256 lds=0 nsplit=8 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=8',
        '=> split=0 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_ncu64': [
        'C 10300000000 rows=2048 cols=512 ld=640',
        'T tns grid=64 block=512 lds=98304 nsplit=4 part=0 colpart=0',
        '=> split=1 shares=4 nonempty=4 floats=8404992',
    ],
    'tn_row_stride_ncu64_ordered': [
        'T tns_part grid=128 block=512 lds=98304 nsplit=8 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=8',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_ncu304': [
        'C 10300000000 rows=2048 cols=512 ld=640',
        'T tn grid=512 block=256 lds=0 nsplit=8 part=0 colpart=0',
        '=> split=0 shares=8 nonempty=8 floats=8404992',
    ],
    'tn_row_stride_ncu304_ordered': [
        'T tns_part grid=128 block=512 lds=98304 nsplit=8 part=10400000000 colpart=10402000000',
        'R grid=2048 nz=8',
        '=> split=1 shares=8 nonempty=8 floats=8404992',
    ],
}

# ---- tests/test_gpu_lstm_gemm.py: every case of tests/lstm_gemm_cases.py under every option setting it runs with (the lines equal
# lstm_gemm_cases.plan_line: tests/test_lstm_gemm_cases.py), and what the planner refuses: side outputs as 256x256 tiles ----
for _line in '''\
G lstm_a_bias_tile0_step2 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_bias_tile1_step2 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_bias_tile2_step2 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_bias_split1_step2 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_bias_split2_image_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1
G lstm_a_bias_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_nobias_tile0_step2 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_nobias_tile1_step2 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_nobias_tile2_step2 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_nobias_split1_step2 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_a_nobias_split2_image_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1
G lstm_a_nobias_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_b_step_plus_tile0_step3 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_plus_tile1_step3 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_plus_tile2_step3 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_plus_split1_step3 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_plus_split2_image_step3 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1 bstatic=1
G lstm_b_step_plus_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_minus_tile0_step3 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_minus_tile1_step3 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_minus_tile2_step3 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_minus_split1_step3 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_b_step_minus_split2_image_step3 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1 bstatic=1
G lstm_b_step_minus_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=3 crows=1
G lstm_c_skip_first_tile0_step0 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=0 crows=1
G lstm_c_skip_first_tile0_step1 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=1 crows=1
G lstm_c_skip_first_tile1_step0 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=0 crows=1
G lstm_c_skip_first_tile1_step1 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=1 crows=1
G lstm_c_skip_first_tile2_step0 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=0 crows=1
G lstm_c_skip_first_tile2_step1 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=1 crows=1
G lstm_c_skip_first_split1_step0 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=0 crows=1
G lstm_c_skip_first_split1_step1 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=1 crows=1
G lstm_c_skip_first_split2_image_step0 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=0 crows=1 bstatic=1
G lstm_c_skip_first_split2_image_step1 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=1 crows=1 bstatic=1
G lstm_c_skip_first_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=0 crows=1
G lstm_c_skip_first_split2_staging_step1 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=2 step=1 crows=1
G lstm_c_first_base_tile0_step0 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=0 crows=1
G lstm_c_first_base_tile0_step1 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=1 crows=1
G lstm_c_first_base_tile1_step0 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=0 crows=1
G lstm_c_first_base_tile1_step1 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=1 crows=1
G lstm_c_first_base_tile2_step0 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=0 crows=1
G lstm_c_first_base_tile2_step1 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=1 crows=1
G lstm_c_first_base_split1_step0 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=0 crows=1
G lstm_c_first_base_split1_step1 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=1 crows=1
G lstm_c_first_base_split2_image_step0 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=0 crows=1 bstatic=1
G lstm_c_first_base_split2_image_step1 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=1 crows=1 bstatic=1
G lstm_c_first_base_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=0 crows=1
G lstm_c_first_base_split2_staging_step1 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=2 skip=0 step=1 crows=1
G lstm_d_two_jobs_tile0_step2 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_two_jobs_tile1_step2 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_two_jobs_tile2_step2 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_two_jobs_split1_step2 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_two_jobs_split2_image_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1
G lstm_d_two_jobs_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_plain_rider_tile0_step2 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1
G lstm_d_plain_rider_tile1_step2 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1
G lstm_d_plain_rider_tile2_step2 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1
G lstm_d_plain_rider_split1_step2 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1
G lstm_d_plain_rider_split2_image_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 bstatic=1
G lstm_d_plain_rider_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1
G lstm_d_four_jobs_tile0_step2 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 ; M=44 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_four_jobs_tile1_step2 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 ; M=44 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_four_jobs_tile2_step2 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 ; M=44 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_four_jobs_split1_step2 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 ; M=44 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_d_four_jobs_split2_image_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 bstatic=1 ; M=44 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 bstatic=1
G lstm_d_four_jobs_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=130 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 ; M=200 N=96 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=2 epiplain=1 ; M=44 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1
G lstm_e_straddle_dead_tile0_step2 epi=1 tile=0 arith=0 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_dead_tile1_step2 epi=1 tile=1 arith=0 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_dead_tile2_step2 epi=1 tile=2 arith=0 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_dead_split1_step2 epi=1 tile=-1 arith=1 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_dead_split2_image_step2 epi=1 tile=-1 arith=2 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48 bstatic=1
G lstm_e_straddle_dead_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_live_tile0_step2 epi=1 tile=0 arith=0 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_live_tile1_step2 epi=1 tile=1 arith=0 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_live_tile2_step2 epi=1 tile=2 arith=0 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_live_split1_step2 epi=1 tile=-1 arith=1 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_straddle_live_split2_image_step2 epi=1 tile=-1 arith=2 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48 bstatic=1
G lstm_e_straddle_live_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=384 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=48
G lstm_e_finished_lines_tile0_step2 epi=1 tile=0 arith=0 ; M=1024 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=256
G lstm_e_finished_lines_tile1_step2 epi=1 tile=1 arith=0 ; M=1024 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=256
G lstm_e_finished_lines_tile2_step2 epi=1 tile=2 arith=0 ; M=1024 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=256
G lstm_e_finished_lines_split1_step2 epi=1 tile=-1 arith=1 ; M=1024 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=256
G lstm_e_finished_lines_split2_image_step2 epi=1 tile=-1 arith=2 ; M=1024 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=256 bstatic=1
G lstm_e_finished_lines_split2_staging_step2 epi=1 tile=-1 arith=2 ; M=1024 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 nact=256
G lstm_f_side_outputs_tile0_step2 epi=1 tile=0 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 zinit=1 gates=1 out2=1
G lstm_f_side_outputs_tile1_step2 epi=1 tile=1 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 zinit=1 gates=1 out2=1
G lstm_f_side_outputs_tile2_step2 epi=1 tile=2 arith=0 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 zinit=1 gates=1 out2=1
G lstm_p_plain_launch_tile0_step2 epi=0 tile=0 arith=0 ; M=300 N=200 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2
G lstm_p_plain_launch_tile1_step2 epi=0 tile=1 arith=0 ; M=300 N=200 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2
G lstm_p_plain_launch_tile2_step2 epi=0 tile=2 arith=0 ; M=300 N=200 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2
G lstm_p_plain_launch_split1_step2 epi=0 tile=-1 arith=1 ; M=300 N=200 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2
G lstm_p_plain_launch_split2_image_step2 epi=0 tile=-1 arith=2 ; M=300 N=200 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 bstatic=1
G lstm_p_plain_launch_split2_staging_step2 epi=0 tile=-1 arith=2 ; M=300 N=200 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2
G lstm_s_8448_split1_step0 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1
G lstm_s_8448_split1_step3 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1
G lstm_s_8448_split2_image_step0 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 bstatic=1
G lstm_s_8448_split2_image_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 bstatic=1
G lstm_s_8448_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1
G lstm_s_8448_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1
G lstm_s_8492_split1_step0 epi=1 tile=-1 arith=1 ; M=8492 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1
G lstm_s_8492_split1_step3 epi=1 tile=-1 arith=1 ; M=8492 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1
G lstm_s_8492_split2_image_step0 epi=1 tile=-1 arith=2 ; M=8492 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 bstatic=1
G lstm_s_8492_split2_image_step3 epi=1 tile=-1 arith=2 ; M=8492 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 bstatic=1
G lstm_s_8492_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=8492 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1
G lstm_s_8492_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=8492 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1
G lstm_s_8192_lines_of_8_split1_step0 epi=1 tile=-1 arith=1 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 nact=8
G lstm_s_8192_lines_of_8_split1_step3 epi=1 tile=-1 arith=1 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 nact=8
G lstm_s_8192_lines_of_8_split2_image_step0 epi=1 tile=-1 arith=2 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 nact=8 bstatic=1
G lstm_s_8192_lines_of_8_split2_image_step3 epi=1 tile=-1 arith=2 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 nact=8 bstatic=1
G lstm_s_8192_lines_of_8_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 nact=8
G lstm_s_8192_lines_of_8_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 nact=8
G lstm_s_8448_lines_of_8_split1_step0 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 nact=8
G lstm_s_8448_lines_of_8_split1_step3 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 nact=8
G lstm_s_8448_lines_of_8_split2_image_step0 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 nact=8 bstatic=1
G lstm_s_8448_lines_of_8_split2_image_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 nact=8 bstatic=1
G lstm_s_8448_lines_of_8_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=0 crows=1 nact=8
G lstm_s_8448_lines_of_8_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 nact=8
G lstm_s_first_base_split1_step0 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=2 skip=0 step=0 crows=1
G lstm_s_first_base_split1_step3 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=2 skip=0 step=3 crows=1
G lstm_s_first_base_split2_image_step0 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=2 skip=0 step=0 crows=1 bstatic=1
G lstm_s_first_base_split2_image_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=2 skip=0 step=3 crows=1 bstatic=1
G lstm_s_first_base_split2_staging_step0 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=2 skip=0 step=0 crows=1
G lstm_s_first_base_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=2 skip=0 step=3 crows=1
G lstm_s_step_split1_step3 epi=1 tile=-1 arith=1 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=0 step=3 crows=1 ; M=8192 N=1024 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=3 epiplain=1
G lstm_s_step_split2_image_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=0 step=3 crows=1 bstatic=1 ; M=8192 N=1024 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=3 epiplain=1 bstatic=1
G lstm_s_step_split2_staging_step3 epi=1 tile=-1 arith=2 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=0 step=3 crows=1 ; M=8192 N=1024 segs=64 koffs=16 lds=96 Ktot=96 rows=1 first=0 skip=0 step=3 epiplain=1
G lstm_s_8448_split2_image_ncu304 epi=1 tile=-1 arith=2 ncu=304 ; M=8448 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 Ktot=160 rows=3 first=0 skip=2 step=3 crows=1 bstatic=1
G lstm_f_side_outputs_split1 epi=1 tile=-1 arith=1 ; M=300 N=256 segs=32,64,32 koffs=96,32,0 lds=64,96,64 Ktot=128 rows=3 first=0 skip=0 step=2 crows=1 zinit=1 gates=1 out2=1
G lstm_chip_filling_split2 epi=1 arith=2 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 rows=3 crows=1 bstatic=1
G lstm_side_outputs_chip_filling_split2 epi=1 arith=2 ; M=8192 N=2048 segs=64,64,32 koffs=96,32,0 lds=96,96,64 rows=3 crows=1 bstatic=1 zinit=1 gates=1 out2=1
'''.splitlines():
    CASES.append((_line.split()[1], _line))

EXPECTED.update({
    'lstm_a_bias_tile0_step2': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_bias_tile1_step2': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_bias_tile2_step2': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_bias_split1_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_bias_split2_image_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_bias_split2_staging_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_nobias_tile0_step2': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_nobias_tile1_step2': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_nobias_tile2_step2': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_nobias_split1_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_nobias_split2_image_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_a_nobias_split2_staging_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_plus_tile0_step3': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_plus_tile1_step3': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_plus_tile2_step3': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_plus_split1_step3': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_plus_split2_image_step3': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_plus_split2_staging_step3': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_minus_tile0_step3': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_minus_tile1_step3': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_minus_tile2_step3': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_minus_split1_step3': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_minus_split2_image_step3': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_b_step_minus_split2_staging_step3': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_tile0_step0': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_tile0_step1': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_tile1_step0': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_tile1_step1': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_tile2_step0': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_tile2_step1': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_split1_step0': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_split1_step1': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_split2_image_step0': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_split2_image_step1': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_split2_staging_step0': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_skip_first_split2_staging_step1': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_tile0_step0': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_tile0_step1': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_tile1_step0': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_tile1_step1': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_tile2_step0': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_tile2_step1': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_split1_step0': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_split1_step1': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_split2_image_step0': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_split2_image_step1': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_split2_staging_step0': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_c_first_base_split2_staging_step1': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_two_jobs_tile0_step2': [
        'L g128 epi=1 grid=6,2,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_two_jobs_tile1_step2': [
        'L k32 epi=1 grid=20,2,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_two_jobs_tile2_step2': [
        'L k64 epi=1 grid=10,2,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_two_jobs_split1_step2': [
        'L s128 epi=1 grid=6,2,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_two_jobs_split2_image_step2': [
        'L s128 epi=1 grid=6,2,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_two_jobs_split2_staging_step2': [
        'L s128 epi=1 grid=6,2,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_plain_rider_tile0_step2': [
        'L g128 epi=1 grid=6,2,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_plain_rider_tile1_step2': [
        'L k32 epi=1 grid=20,2,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_plain_rider_tile2_step2': [
        'L k64 epi=1 grid=10,2,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_plain_rider_split1_step2': [
        'L s128 epi=1 grid=6,2,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_plain_rider_split2_image_step2': [
        'L s128 epi=1 grid=6,2,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_plain_rider_split2_staging_step2': [
        'L s128 epi=1 grid=6,2,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_four_jobs_tile0_step2': [
        'L g128 epi=1 grid=6,4,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=30100000000/30800000000/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=44 N=256 ks=0 xcd=0 ep=0 a0=40100000000/40800000000/0 a1=40200000000/40900000000/0 a2=40300000000/0/0 c=40400000000/40500000000/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_four_jobs_tile1_step2': [
        'L k32 epi=1 grid=20,4,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=30100000000/30800000000/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=44 N=256 ks=0 xcd=0 ep=0 a0=40100000000/40800000000/0 a1=40200000000/40900000000/0 a2=40300000000/0/0 c=40400000000/40500000000/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_four_jobs_tile2_step2': [
        'L k64 epi=1 grid=10,4,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=30100000000/30800000000/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=44 N=256 ks=0 xcd=0 ep=0 a0=40100000000/40800000000/0 a1=40200000000/40900000000/0 a2=40300000000/0/0 c=40400000000/40500000000/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_four_jobs_split1_step2': [
        'L s128 epi=1 grid=6,4,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=30100000000/30800000000/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=44 N=256 ks=0 xcd=0 ep=0 a0=40100000000/40800000000/0 a1=40200000000/40900000000/0 a2=40300000000/0/0 c=40400000000/40500000000/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_four_jobs_split2_image_step2': [
        'L s128 epi=1 grid=6,4,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=30100000000/30800000000/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=44 N=256 ks=0 xcd=0 ep=0 a0=40100000000/40800000000/0 a1=40200000000/40900000000/0 a2=40300000000/0/0 c=40400000000/40500000000/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_d_four_jobs_split2_staging_step2': [
        'L s128 epi=1 grid=6,4,1 block=256 lds=77824 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=130 N=256 ks=0 xcd=0 ep=0 a0=20100000000/20800000000/0 a1=20200000000/20900000000/0 a2=20300000000/0/0 c=20400000000/20500000000/0 o=21000000000 co=21100000000 z=0 go=0 o2=0 na=0 | M=200 N=96 ks=0 xcd=0 ep=1 a0=30100000000/30800000000/0 c=0/0/0 o=31000000000 co=0 z=0 go=0 o2=0 na=0 | M=44 N=256 ks=0 xcd=0 ep=0 a0=40100000000/40800000000/0 a1=40200000000/40900000000/0 a2=40300000000/0/0 c=40400000000/40500000000/0 o=41000000000 co=41100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_e_straddle_dead_tile0_step2': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_dead_tile1_step2': [
        'L k32 epi=1 grid=24,1,1 block=256 lds=0 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_dead_tile2_step2': [
        'L k64 epi=1 grid=12,1,1 block=256 lds=0 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_dead_split1_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_dead_split2_image_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_dead_split2_staging_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_live_tile0_step2': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_live_tile1_step2': [
        'L k32 epi=1 grid=24,1,1 block=256 lds=0 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_live_tile2_step2': [
        'L k64 epi=1 grid=12,1,1 block=256 lds=0 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_live_split1_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_live_split2_image_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_straddle_live_split2_staging_step2': [
        'L s128 epi=1 grid=6,1,1 block=256 lds=77824 img=0/0 | M=384 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_finished_lines_tile0_step2': [
        'L g128 epi=1 grid=16,1,1 block=256 lds=69632 img=0/0 | M=1024 N=256 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_finished_lines_tile1_step2': [
        'L k32 epi=1 grid=64,1,1 block=256 lds=0 img=0/0 | M=1024 N=256 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_finished_lines_tile2_step2': [
        'L k64 epi=1 grid=32,1,1 block=256 lds=0 img=0/0 | M=1024 N=256 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_finished_lines_split1_step2': [
        'L s128 epi=1 grid=16,1,1 block=256 lds=77824 img=0/0 | M=1024 N=256 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_finished_lines_split2_image_step2': [
        'L s128 epi=1 grid=16,1,1 block=256 lds=77824 img=0/0 | M=1024 N=256 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_e_finished_lines_split2_staging_step2': [
        'L s128 epi=1 grid=16,1,1 block=256 lds=77824 img=0/0 | M=1024 N=256 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_f_side_outputs_tile0_step2': [
        'L g128 epi=1 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
    'lstm_f_side_outputs_tile1_step2': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
    'lstm_f_side_outputs_tile2_step2': [
        'L k64 epi=1 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
    'lstm_p_plain_launch_tile0_step2': [
        'L g128 epi=0 grid=6,1,1 block=256 lds=69632 img=0/0 | M=300 N=200 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_p_plain_launch_tile1_step2': [
        'L k32 epi=0 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=200 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_p_plain_launch_tile2_step2': [
        'L k64 epi=0 grid=10,1,1 block=256 lds=0 img=0/0 | M=300 N=200 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_p_plain_launch_split1_step2': [
        'L s128 epi=0 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=200 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_p_plain_launch_split2_image_step2': [
        'L s128 epi=0 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=200 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_p_plain_launch_split2_staging_step2': [
        'L s128 epi=0 grid=6,1,1 block=256 lds=77824 img=0/0 | M=300 N=200 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=0/0/0 o=11000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split1_step0': [
        'L s128 epi=1 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split1_step3': [
        'L s128 epi=1 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split2_image_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split2_image_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split2_staging_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split2_staging_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8492_split1_step0': [
        'L s128 epi=1 grid=1072,1,1 block=256 lds=77824 img=0/0 | M=8492 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8492_split1_step3': [
        'L s128 epi=1 grid=1072,1,1 block=256 lds=77824 img=0/0 | M=8492 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8492_split2_image_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8492_split2_image_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8492_split2_staging_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8492_split2_staging_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=48,1,1 block=256 lds=77824 img=0/0 | M=300 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8192_lines_of_8_split1_step0': [
        'L s128 epi=1 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8192_lines_of_8_split1_step3': [
        'L s128 epi=1 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8192_lines_of_8_split2_image_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8192_lines_of_8_split2_image_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8192_lines_of_8_split2_staging_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8192_lines_of_8_split2_staging_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8448_lines_of_8_split1_step0': [
        'L s128 epi=1 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8448_lines_of_8_split1_step3': [
        'L s128 epi=1 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
    ],
    'lstm_s_8448_lines_of_8_split2_image_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500001000',
    ],
    'lstm_s_8448_lines_of_8_split2_image_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500001000',
    ],
    'lstm_s_8448_lines_of_8_split2_staging_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500001000',
    ],
    'lstm_s_8448_lines_of_8_split2_staging_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=11500000000',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=11500001000',
    ],
    'lstm_s_first_base_split1_step0': [
        'L s128 epi=1 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_first_base_split1_step3': [
        'L s128 epi=1 grid=1056,1,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_first_base_split2_image_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/10d00300000 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_first_base_split2_image_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/10d00300000 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_first_base_split2_staging_step0': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/10d00300000 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_first_base_split2_staging_step3': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/10d00000000 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/10d00300000 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_step_split1_step3': [
        'L s128 epi=1 grid=1056,2,1 block=256 lds=77824 img=0/0 | M=8448 N=2048 ks=0 xcd=2 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=8192 N=1024 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_step_split2_image_step3': [
        'L s256 epi=1 grid=256,2,1 block=512 lds=163840 img=1/2 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=8192 N=1024 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_step_split2_staging_step3': [
        'L s256 epi=1 grid=256,2,1 block=512 lds=163840 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0 | M=8192 N=1024 ks=0 xcd=0 ep=1 a0=20100000000/20800000000/0 c=0/0/0 o=21000000000 co=0 z=0 go=0 o2=0 na=0',
        'L s128 epi=1 grid=32,1,1 block=256 lds=77824 img=0/0 | M=256 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800008000/0 a1=10200000000/10900008000/0 a2=10300200000/0/0 c=10400000000/10500008000/0 o=11001000000 co=11101000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_s_8448_split2_image_ncu304': [
        'L s256 epi=1 grid=264,1,1 block=512 lds=163840 img=1/1 | M=8448 N=2048 ks=0 xcd=1 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_f_side_outputs_split1': [
        'L k32 epi=1 grid=20,1,1 block=256 lds=0 img=0/0 | M=300 N=256 ks=0 xcd=0 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
    'lstm_chip_filling_split2': [
        'L s256 epi=1 grid=256,1,1 block=512 lds=163840 img=1/1 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=0 go=0 o2=0 na=0',
    ],
    'lstm_side_outputs_chip_filling_split2': [
        'L s128 epi=1 grid=1024,1,1 block=256 lds=77824 img=0/0 | M=8192 N=2048 ks=0 xcd=4 ep=0 a0=10100000000/10800000000/0 a1=10200000000/10900000000/0 a2=10300000000/0/0 c=10400000000/10500000000/0 o=11000000000 co=11100000000 z=11200000000 go=11300000000 o2=11400000000 na=0',
    ],
})
