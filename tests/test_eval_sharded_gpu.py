"""Sharded evaluation under P3D_DEVICE_EVAL=1: two processes (gloo over the one card of the test box, as tests/test_ddp_gpu.py) run
Trainer.test on 3 and on 4 test batches.  Each rank must run the forward for exactly its batches i = rank (mod 2) and both must return a
record bit-equal to the single-process record with the switch on; also through the synthetic test loader, which loads only the rank's batches."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden_path

pytestmark = pytest.mark.gpu

COUNTS = (3, 4)


def _trainer(pkg, meta):
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128', '-metadata', meta, '-synthetic', '3', '-batch_size', '2', '-workers', '0'])
    model, _ = pkg.depth_main.create_model(args)
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
    trainer.verbose = False
    seen = []
    infer = trainer.vanilla_infer

    def counted(image, i_batch=0, ret_last=False):
        seen.append(i_batch)
        return infer(image, i_batch, ret_last)

    trainer.vanilla_infer = counted
    return args, trainer, seen


def _batches(pkg, n):
    out = []
    for it in range(n):
        c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=3, step=it, invalid_frac=0.25)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(50 + it)).standard_normal((2, 3, 3)))[0].astype(np.float32)
        out.append(tuple(torch.from_numpy(a) for a in (c, d, tc, tv, rot)))
    return out


def _run_all(pkg, meta):
    """{name: (record, batches whose forward ran)} for the lists of COUNTS batches and the synthetic test loader."""
    args, trainer, seen = _trainer(pkg, meta)
    out = {}
    for n in COUNTS:
        del seen[:]
        out['list%d' % n] = (trainer.test(1, _batches(pkg, n)), list(seen))
    del seen[:]
    loader = pkg.depth_datasets.data_loader(args, 'test', pkg.utils.get_info())
    out['loader'] = (trainer.test(1, loader), list(seen))
    return out


def _worker(rank, world, port, pkg_name, meta, out_dir):
    import importlib
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      P3D_DIST_BACKEND='gloo', P3D_DEVICE_EVAL='1')
    pkg = importlib.import_module(pkg_name)
    pkg.dist.init_from_env()
    out = _run_all(pkg, meta)
    torch.save(out, os.path.join(out_dir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_split_the_test_batches_and_agree(pkg, tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    port = 29300 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(2, port, pkg.__name__, str(meta), str(tmp_path)), nprocs=2, join=True)
    ranks = [torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r)) for r in (0, 1)]

    for key in ('WORLD_SIZE', 'RANK'):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '1')
    single = _run_all(pkg, str(meta))
    for name, (record, seen) in single.items():
        n = len(seen)
        assert seen == list(range(n)), name
        for rank, got in enumerate(ranks):
            got_record, got_seen = got[name]
            assert got_seen == list(range(rank, n, 2)), (name, rank, got_seen)
            assert got_record == record, (name, rank, got_record, record)            # bit-equal: the same float values, key by key
    assert len(single['list3'][1]) == 3 and len(single['list4'][1]) == 4 and len(single['loader'][1]) == 3
