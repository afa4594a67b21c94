"""The configuration bench.py measures, pinned end to end against the CPU oracle (VERDICT r2 "weak" 1, 3):

  * one SUGStep.step with bench.BENCH_METHODS (SOFT_MMD on both levels, GEO_WEIGHTS and SEM_WEIGHTS 'mean2one',
    tools/cfgs/cfgs_local/DG_unified_loss.yaml) against oracle.sug_losses under the same METHODS at 1e-4 -- launched
    eagerly, replayed from the captured hipGraph, and with the tuned GEMM table -- at B=8 and at the benched B=32;
  * mmd.mmd_cal(..., GEO_WEIGHTS='mean2one', data_s, data_t) against oracle.mmd_cal (train_dg_single_gpu.py:314,
    model/mmd.py:107-131, :178-202);
  * the steps of BASELINE configs 3 and 5 at their per-GPU sizes (PointNet++ 64 x 2048; Point Transformer 16 x 2048 in its
    fp16 mode): finite, reproducible, and for config 5 the deviation of the fp16 mode from fp32 reported and bounded;
  * a plain `bench.py` run (no --full): the headline line and nothing measured after the timed steps.
"""
import pytest
import torch

import bench
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _batch(B, N, seed=11):
    g = torch.Generator().manual_seed(seed)
    data, data_t = O.synth_clouds(B, N, g), O.synth_clouds(B, N, g)
    lab, lab_t = torch.randint(0, 10, (B,), generator=g), torch.randint(0, 10, (B,), generator=g)
    return data, lab, data_t, lab_t


def _oracle_losses(B, N=1024, wseed=5, sseed=21):
    """oracle.sug_losses under bench.BENCH_METHODS (forward only), cached per batch size."""
    key = (B, N, wseed, sseed)
    if key not in _ORACLE:
        from sug_amd.model.Model import Net_MDA
        shapes = {k: tuple(v.shape) for k, v in Net_MDA('DGCNN').state_dict().items()}
        p = O.as_params(O.fill_params(shapes, wseed))
        data, lab, data_t, lab_t = _batch(B, N)
        torch.manual_seed(sseed)                   # FPS start draws: sem-s, sem-t, node-s, node-t (reference call order)
        with torch.no_grad():
            lc, lg, ls = O.sug_losses(p, 'DGCNN', data, lab, data_t, lab_t, dict(bench.BENCH_METHODS['GEO_MMD'][0]),
                                      dict(bench.BENCH_METHODS['SEM_MMD'][0]), drop_p=0.0)
        _ORACLE[key] = [float(lc), float(lg), float(ls)]
    return _ORACLE[key]


def _trainer(B, use_graph, tuned, wseed=5, lr=0.0, model_name='DGCNN', single_pass=False):
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    net = Net_MDA(model_name)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, wseed))
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    if tuned:
        from sug_amd.tuning import enable_tuned_gemms
        enable_tuned_gemms()
    # lr = 0: Adam leaves the weights where they are, so the planning step, the captured step and every replay see
    # the same weights and each of them can be held against the one oracle evaluation
    return SUGStep(net.cuda().train(), lr=lr, weight_decay=5e-5, use_graph=use_graph, methods=bench.BENCH_METHODS,
                   single_pass=single_pass)


def _untune():
    import torch.cuda.tunable as tn
    from sug_amd import ops
    tn.enable(False)
    ops.DW_FORCE_LIBRARY = False
    ops.DW_LIBRARY_SHAPES = set()


@pytest.mark.parametrize('mode', ['eager', 'graph', 'eager_tuned', 'graph_tuned'])
def test_bench_methods_step_matches_oracle(mode):
    """B = 8, dropout 0: (loss_cls, loss_geo_mmd, loss_sem_mmd) of SUGStep.step under bench.BENCH_METHODS == the
    oracle's within 1e-4; in graph mode for the eager planning step, the captured step and two replays alike."""
    B = 8
    want = _oracle_losses(B)
    data, lab, data_t, lab_t = [t.cuda() for t in _batch(B, 1024)]
    try:
        tr = _trainer(B, mode.startswith('graph'), mode.endswith('tuned'))
        assert tr.methods['GEO_MMD'][0]['GEO_WEIGHTS'] == 'mean2one' and tr.methods['SEM_MMD'][0]['SEM_WEIGHTS'] == 'mean2one'
        got = []
        for _ in range(4 if tr.use_graph else 2):
            torch.manual_seed(21)
            got.append([float(v) for v in tr.step(data, lab, data_t, lab_t)])
        if tr.use_graph:
            assert len(tr._graphs) == 1 and next(iter(tr._graphs.values()))['graph'] is not None
    finally:
        _untune()
    print(mode, 'gpu', got, 'oracle', want)
    for step in got:
        for a, b in zip(step, want):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (mode, got, want)


def test_benched_configuration_b32_graph_tuned_matches_oracle():
    """Exactly what `python bench.py` times (DGCNN, 32 clouds per domain, N=1024, BENCH_METHODS, hipGraph replay,
    tuned GEMM table, own weight-gradient kernels under capture) except dropout: the replayed step's three losses
    against the oracle's at 1e-4."""
    B = 32
    want = _oracle_losses(B)
    data, lab, data_t, lab_t = [t.cuda() for t in _batch(B, 1024)]
    try:
        tr = _trainer(B, True, True)
        got = []
        for _ in range(3):
            torch.manual_seed(21)
            got.append([float(v) for v in tr.step(data, lab, data_t, lab_t)])
    finally:
        _untune()
    print('gpu', got, 'oracle', want)
    for step in got:
        for a, b in zip(step, want):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)


def test_benched_configuration_b32_single_pass_graph_tuned_matches_oracle_with_tied_starts():
    """`bench.py`'s config.single_pass_ms_per_step configuration (DGCNN, 32 clouds per domain, hipGraph replay, tuned GEMMs,
    SUGStep(single_pass=True)) except dropout: planning step, captured step and a replay against oracle.sug_losses whose
    node passes draw the semantic passes' FPS starts, at 1e-4.  The step makes ONE draw of 2B starts per sampling stage
    (source clouds first), which is the tie handed to the oracle."""
    from sug_amd.model.Model import Net_MDA
    B, N = 32, 1024
    batch = _batch(B, N)
    data, lab, data_t, lab_t = [t.cuda() for t in batch]
    torch.manual_seed(21)
    d = torch.randint(0, N, (2 * B,), dtype=torch.long)
    s_s, s_t = [d[:B]], [d[B:]]
    p = O.as_params(O.fill_params({k: tuple(v.shape) for k, v in Net_MDA('DGCNN').state_dict().items()}, 5))
    with torch.no_grad():
        want = [float(v) for v in O.sug_losses(p, 'DGCNN', batch[0], batch[1], batch[2], batch[3],
                                               dict(bench.BENCH_METHODS['GEO_MMD'][0]), dict(bench.BENCH_METHODS['SEM_MMD'][0]),
                                               drop_p=0.0, starts=[s_s, s_t, s_s, s_t])]
    try:
        tr = _trainer(B, True, True, single_pass=True)
        got = []
        for _ in range(3):
            torch.manual_seed(21)
            got.append([float(v) for v in tr.step(data, lab, data_t, lab_t)])
        assert len(tr._graphs) == 1 and next(iter(tr._graphs.values()))['graph'] is not None
    finally:
        _untune()
    print('single pass gpu', got, 'oracle (tied starts)', want)
    for step in got:
        for a, b in zip(step, want):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)


@pytest.mark.parametrize('weighting', ['mean2one', 'none', 'naive_inverse', 'exp_inverse'])
def test_mmd_cal_with_geometric_weights_matches_oracle(weighting):
    """mmd_cal on node features with GEO_WEIGHTS (Chamfer distance of the paired clouds -> distance2weights ->
    weighted K_XY column sums), value and gradient, against oracle.mmd_cal (fp32) -- the first MMD term of a step,
    train_dg_single_gpu.py:314."""
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(31)
    m, D, N = 8, 4096, 1024
    fs = (torch.randn(m, D, generator=g) * 0.3).requires_grad_(True)
    ft = (torch.randn(m, D, generator=g) * 0.3 + 0.05).requires_grad_(True)
    ls, lt = torch.randint(0, 10, (m,), generator=g), torch.randint(0, 10, (m,), generator=g)
    ds, dt = O.synth_clouds(m, N, g), O.synth_clouds(m, N, g)
    cfg = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 50, 'GEO_WEIGHTS': weighting, 'GEO_SCALE': 1}
    with torch.no_grad():
        want = O.mmd_cal(ls, fs, lt, ft, cfg, ds, dt)
    # gradient reference in fp64: the reference's own fp32 autograd gradient of the MMD is cancellation noise
    # (tests/test_gpu_mmd.py); the weights enter as fp32 values on both sides
    fd, td = fs.detach().double().requires_grad_(True), ft.detach().double().requires_grad_(True)
    w64 = O.chamfer_weights(ds, dt, weighting).double()
    gw = torch.autograd.grad(O.soft_mmd(ls, fd, lt, td, float(cfg['LABEL_SCALE']), w64), (fd, td))
    fsg, ftg = fs.detach().cuda().requires_grad_(True), ft.detach().cuda().requires_grad_(True)
    got = mmd.mmd_cal(ls.cuda(), fsg, lt.cuda(), ftg, cfg, data_s=ds.cuda(), data_t=dt.cuda())
    gg = torch.autograd.grad(got, (fsg, ftg))
    w_ref = O.chamfer_weights(ds, dt, weighting).reshape(-1)
    w_gpu = mmd.geometric_weights(ds.cuda(), dt.cuda(), weighting=weighting).reshape(-1).cpu()
    torch.testing.assert_close(w_gpu, w_ref, rtol=1e-4, atol=1e-6)
    assert abs(float(got.detach()) - float(want)) <= 1e-4 * max(1.0, abs(float(want))), (float(got.detach()), float(want))
    s = max(float(g.abs().max()) for g in gw)
    for a, b in zip(gg, gw):
        torch.testing.assert_close(a.cpu().double(), b, rtol=1e-3, atol=2e-4 * s)


def test_config3_step_at_full_batch():
    """BASELINE config 3 at its full per-GPU size (PointNet++, 64 clouds per domain, N=2048): two steps, finite
    losses, run-to-run reproducible first step (float atomics only in small scatter kernels)."""
    B, N = 64, 2048
    data, lab, data_t, lab_t = [t.cuda() for t in _batch(B, N, seed=13)]
    res = []
    for _ in range(2):
        tr = _trainer(B, False, False, lr=1e-3, model_name='Pointnet2')
        torch.manual_seed(77)
        res.append([[float(v) for v in tr.step(data, lab, data_t, lab_t)] for _ in range(2)])
        del tr
        torch.cuda.empty_cache()
    print(res)
    for run in res:
        for step in run:
            assert all(v == v and abs(v) < 1e4 for v in step), res
    for a, b in zip(res[0][0], res[1][0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), res
    assert res[0][1] != res[0][0], 'the Adam updates must move the losses'


def test_config5_fp16_step_at_full_per_gpu_share():
    """BASELINE config 5's per-GPU share (Point Transformer, 16 clouds per domain, N=2048) in its fp16 mode
    (k-expanded attention tensors and every 512-wide linear of the blocks on the fp16 MFMA path, fp32 accumulation):
    finite, reproducible to the library GEMMs' run-to-run noise, and within 2e-2 of the fp32 step's losses (the
    reference arithmetic; the deviation is printed)."""
    from sug_amd.model import Ptran_transformer as PT
    B, N = 16, 2048
    data, lab, data_t, lab_t = [t.cuda() for t in _batch(B, N, seed=17)]
    out = {}
    try:
        for name, dt in (('fp32', None), ('fp16', torch.float16), ('fp16_again', torch.float16)):
            PT.GEMM_DTYPE, PT.PROJ_16BIT = dt, dt is not None
            tr = _trainer(B, False, False, lr=1e-3, model_name='PTran')
            torch.manual_seed(77)
            out[name] = [[float(v) for v in tr.step(data, lab, data_t, lab_t)] for _ in range(2)]
            del tr
            torch.cuda.empty_cache()
    finally:
        PT.GEMM_DTYPE, PT.PROJ_16BIT = None, False
    print(out)
    for run in out.values():
        for step in run:
            assert all(v == v and abs(v) < 1e4 for v in step), out
    dev = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(out['fp16'][0], out['fp32'][0]))
    rep = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(out['fp16'][0], out['fp16_again'][0]))
    print('config 5 first-step losses: fp16 vs fp32 deviation %.3e, fp16 run-to-run %.3e' % (dev, rep))
    assert dev <= 2e-2, out
    assert rep <= 2e-3, out


# ---- round 6: configs 3 and 5 at their FULL per-GPU sizes against the oracle, not by properties only --------
_FULL = {'Pointnet2': (64, 2048, 13), 'PTran': (16, 2048, 17)}          # model -> (clouds per domain, N, batch seed)


def _fps_counts(model_name, N):
    return {'Pointnet2': (N, 512), 'PTran': (N, 256, 64, 16)}[model_name]


def _full_size_oracle(model_name, tied):
    """oracle.sug_losses (forward only, dropout 0, fp32) at the benched size under bench.BENCH_METHODS.  tied=False: the four
    passes draw their FPS starts from the CPU generator seeded 21, in the reference's call order (what the two-pass step
    draws); tied=True: the node passes use the semantic passes' starts (what the single-pass step computes)."""
    key = ('full', model_name, tied)
    if key not in _ORACLE:
        from sug_amd.model.Model import Net_MDA
        B, N, bseed = _FULL[model_name]
        p = O.as_params(O.fill_params({k: tuple(v.shape) for k, v in Net_MDA(model_name).state_dict().items()}, 5))
        data, lab, data_t, lab_t = _batch(B, N, seed=bseed)
        torch.manual_seed(21)
        starts = None
        if tied:
            s_s = tuple(torch.randint(0, n, (B,), dtype=torch.long) for n in _fps_counts(model_name, N))
            s_t = tuple(torch.randint(0, n, (B,), dtype=torch.long) for n in _fps_counts(model_name, N))
            starts = [s_s, s_t, s_s, s_t]
        with torch.no_grad():
            v = O.sug_losses(p, model_name, data, lab, data_t, lab_t, dict(bench.BENCH_METHODS['GEO_MMD'][0]),
                             dict(bench.BENCH_METHODS['SEM_MMD'][0]), drop_p=0.0, starts=starts)
        _ORACLE[key] = [float(t) for t in v]
    return _ORACLE[key]


@pytest.mark.parametrize('model_name', ['Pointnet2', 'PTran'])
@pytest.mark.parametrize('single_pass', [False, True])
def test_configs_3_and_5_full_size_graph_tuned_match_oracle(model_name, single_pass):
    """BASELINE config 3 (PointNet++, 64 clouds per domain, N = 2048) and config 5's per-GPU share (Point Transformer, 16 clouds
    per domain, N = 2048, fp32 = the reference arithmetic) in the launch mode bench.py times -- hipGraph replay, tuned GEMM
    table -- with dropout 0 and lr 0: the three losses of the planning step, the captured step and a replay against
    oracle.sug_losses at 1e-4; the exact two-pass step (FPS starts drawn in the reference's call order) and the opt-in
    single-pass step (oracle with the node passes' starts tied to the semantic passes')."""
    B, N, bseed = _FULL[model_name]
    want = _full_size_oracle(model_name, single_pass)
    data, lab, data_t, lab_t = [t.cuda() for t in _batch(B, N, seed=bseed)]
    try:
        tr = _trainer(B, True, True, model_name=model_name, single_pass=single_pass)
        got = []
        for _ in range(3):
            torch.manual_seed(21)
            got.append([float(v) for v in tr.step(data, lab, data_t, lab_t)])
        assert len(tr._graphs) == 1 and next(iter(tr._graphs.values()))['graph'] is not None
        tr.drop_graphs()
    finally:
        _untune()
        torch.cuda.empty_cache()
    print(model_name, 'single-pass' if single_pass else 'two-pass', 'gpu', got, 'oracle', want)
    for step in got:
        for a, b in zip(step, want):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (model_name, single_pass, got, want)


def test_plain_bench_run_reports_the_headline_and_measures_nothing_else():
    """`bench.py` without --full: one JSON line with the headline fields, and nothing measured after the timed steps -- no
    kernel timings or roofline, no eager / unchanged-caller / single-pass steps, no other workloads, no one-rank RCCL
    rehearsal, no CPU baseline (all of that is --full's)."""
    import json
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.abspath(bench.__file__), '--gpus', '1', '--steps', '3', '--warmup', '3'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d['metric'] == 'point-clouds/sec (train step, N=1024)' and d['unit'] == 'point-clouds/sec'
    assert d['higher_is_better'] is True and d['dtype'] == 'f32' and d['steps'] == 3 and d['warmup'] == 3
    assert d['value'] > 0 and abs(d['value'] - 64 / (d['ms_per_step'] * 1e-3)) <= 1e-9 * d['value']
    assert d['config']['launch'] == 'hipGraph replay of the whole step'
    assert d['roofline'] is None and d['kernels'] == {} and d['cpu_baseline'] is None
    cfg = d['config']
    for k in ('eager_ms_per_step', 'graph_kernel_ms_per_step', 'unchanged_caller_ms_per_step', 'single_pass_ms_per_step',
              'other_workloads', 'segmented_one_rank_rccl', 'collectives'):
        assert cfg[k] is None, (k, cfg[k])
    assert all(v is not None for v in d['losses']), d['losses']
