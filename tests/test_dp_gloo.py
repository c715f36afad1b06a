"""CPU, world_size=2, gloo: the data-parallel exchange (gnnome_assembly_amd/dp.py).

DP parity contract: the all-reduced flat gradient equals the MEAN of the
single-graph gradients.  The per-graph gradients here come from the CPU oracle (the HIP path
needs a GPU); what is under test is the flat-buffer view logic, the collective and the sharding."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from loop_common import mix_sample, oracle_model_factory


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _graph_grads(rank):
    from gnnome_assembly_amd import synth
    from oracle import gatedgcn_oracle as orc
    src, dst, n = synth.make_graph(300, seed=rank)
    inp = synth.make_inputs(src, dst, n, seed=rank)
    sd = synth.synth_state_dict(32, 2, seed=0)
    p = {k: torch.from_numpy(v).requires_grad_(True) for k, v in sd.items()}
    s = orc.model_forward(p, torch.from_numpy(src), torch.from_numpy(dst), n, torch.from_numpy(inp["e"]),
                          torch.from_numpy(inp["pe"]))
    orc.bce_loss(s, torch.from_numpy(inp["y"]), float(inp["pos_weight"])).backward()
    return sd, {k: v.grad for k, v in p.items()}


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp
    r, w = dp.init_process_group("gloo")
    assert (r, w) == (rank, world)
    sd, grads = _graph_grads(rank)
    model = G.GraphGatedGCNModel(1, 2, 32, 16, 2, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    flat = dp.FlatGradients(model.parameters())
    assert flat.grads.numel() == sum(p.numel() for p in model.parameters()) == flat.flat.numel() - 1
    flat.zero_()
    for k, p in model.named_parameters():
        assert p.grad.data_ptr() >= flat.flat.data_ptr()        # a view of the flat buffer
        p.grad += grads[k]                                       # what autograd's accumulation does
    flat.all_reduce_mean()
    torch.optim.Adam(model.parameters(), lr=1e-3).step()
    np.save(os.path.join(out_dir, f"flat{rank}.npy"), flat.grads.numpy())
    np.save(os.path.join(out_dir, f"w{rank}.npy"), torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_flat_gradient_allreduce_is_mean_of_graph_gradients(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    flats = [np.load(tmp_path / f"flat{r}.npy") for r in range(world)]
    ws = [np.load(tmp_path / f"w{r}.npy") for r in range(world)]
    assert np.array_equal(flats[0], flats[1]) and np.array_equal(ws[0], ws[1])     # replicas stay in sync
    import gnnome_assembly_amd as G
    names = [k for k, _ in G.GraphGatedGCNModel(1, 2, 32, 16, 2, 64, True, 16).named_parameters()]
    per = [_graph_grads(r)[1] for r in range(world)]
    want = torch.cat([sum(g[k] for g in per).reshape(-1) / world for k in names]).numpy()
    assert np.abs(flats[0] - want).max() <= 1e-7 * max(1.0, np.abs(want).max())


def test_shard_graphs():
    from gnnome_assembly_amd import dp
    sizes = [5, 9, 1, 7, 3, 8, 2, 6]
    shards = [dp.shard_graphs(8, r, 4, sizes) for r in range(4)]
    assert sorted(sum(shards, [])) == list(range(8))
    # size-sorted: the graphs of one step (same position in every shard) are neighbours in size
    for step in range(2):
        s = sorted(sizes[sh[step]] for sh in shards)
        assert s[-1] - s[0] <= 4
    assert dp.shard_graphs(5, 1, 2) == [1, 3]


def _uneven_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from gnnome_assembly_amd import dp
    dp.init_process_group("gloo")
    mine = dp.shard_graphs(3, rank, world)             # rank 0: graphs [0, 2], rank 1: graph [1]
    w = torch.nn.Parameter(torch.zeros(4))
    flat = dp.FlatGradients([w])
    nsteps = dp.steps_per_epoch(len(mine))
    seen = []
    for it in range(nsteps):                            # the loop shape of train.train
        flat.zero_()
        if it < len(mine):
            w.grad += float(mine[it] + 1)               # "gradient" of graph g = g + 1
        flat.all_reduce_mean(contributed=it < len(mine))
        seen.append(w.grad.clone().numpy())
    np.save(os.path.join(out_dir, f"uneven{rank}.npy"), np.stack(seen))
    dist.barrier()
    dist.destroy_process_group()


def test_size_sorted_shards_keep_every_rank_busy_on_the_mixed_chromosome_set():
    """BASELINE config 4 (8 GPUs, a mixed chr19 / chr20 / chr21 train set): a step takes as long as its largest graph, so a
    rank's idle fraction in a step is 1 - (its graph's size / the step's largest).  The three chromosomes differ by
    1 : 1.073 : 0.731 (evaluate.py:28-30: 61.7 / 66.2 / 45.1 Mb at the same coverage) and simulated replicas by a few per cent
    (load imbalance, not xGMI, is what limits scaling).  With shard_graphs(sizes=...) -- sort by size, deal
    round-robin -- the W graphs of every step are neighbours in the sorted list: every rank's idle fraction stays below 10 % in
    every step and below 5 % over the epoch; dealt in dataset order the same set leaves ranks up to a third idle."""
    from gnnome_assembly_amd import dp
    rng = np.random.default_rng(5)
    world = 8
    base = {"chr19": 1.0, "chr20": 1.073, "chr21": 0.731}
    sizes = [base[c] * (1.0 + 0.03 * rng.standard_normal()) for c in ("chr19", "chr20", "chr21") for _ in range(8)]   # 24 graphs
    rng.shuffle(sizes)

    def idle(sorted_):
        shards = [dp.shard_graphs(len(sizes), r, world, sizes if sorted_ else None) for r in range(world)]
        assert sorted(i for sh in shards for i in sh) == list(range(len(sizes)))
        steps = len(shards[0])
        assert all(len(sh) == steps for sh in shards)
        per_step = np.array([[sizes[shards[r][k]] for r in range(world)] for k in range(steps)])       # [step, rank]
        worst = float((1.0 - per_step / per_step.max(1, keepdims=True)).max())
        epoch = 1.0 - per_step.sum(0) / per_step.max(1).sum()                                          # per rank over the epoch
        return worst, float(epoch.max())
    w_sorted, e_sorted = idle(True)
    w_plain, e_plain = idle(False)
    print(f"idle fraction, worst rank and step / worst rank over the epoch: size-sorted {w_sorted:.3f} / {e_sorted:.3f}, "
          f"dataset order {w_plain:.3f} / {e_plain:.3f}")
    assert w_sorted < 0.10 and e_sorted < 0.05
    assert w_plain > 0.25


def test_uneven_shards_do_not_hang_and_average_over_contributors(tmp_path):
    """3 graphs on 2 ranks (the rank with the shorter shard used to leave the loop early and meet the
    others in the wrong collective).  Every rank takes max-over-ranks steps; a padding step contributes
    nothing and is not counted in the mean."""
    world = 2
    mp.spawn(_uneven_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    a, b = np.load(tmp_path / "uneven0.npy"), np.load(tmp_path / "uneven1.npy")
    assert a.shape == (2, 4) and np.array_equal(a, b)
    assert np.allclose(a[0], (1 + 2) / 2) and np.allclose(a[1], 3.0)     # step 1: graphs 0 and 1; step 2: graph 2 alone


# ------------------------------------------------------------------------------------------------------------------
# BASELINE config 4 in miniature at the REAL world size: train.train under EIGHT gloo ranks on a 24-graph chr19 / chr20 /
# chr21 mix.  The HIP model needs a GPU; what runs here is the product's LOOP -- sharding, the matched
# collectives, the flat-gradient exchange, epoch reductions, files from rank 0 -- around a CPU stand-in model (the
# package's own module class with its forward routed to the fp32 oracle: test infrastructure, hooks["model_factory"]).
# ------------------------------------------------------------------------------------------------------------------
_CHR = {"chr19": 1.0, "chr20": 1.073, "chr21": 0.731}        # evaluate.py:28-30 (synth.CHR_SCALE)


def _mix24(base_reads=240):
    """24 (reads, seed) pairs: 8 replicas of each chromosome, +-3 % in size, in a shuffled dataset order."""
    rng = np.random.default_rng(5)
    reads = [max(8, int(round(base_reads * _CHR[c] * (1.0 + 0.03 * rng.standard_normal())))) for c in _CHR for _ in range(8)]
    order = rng.permutation(len(reads))
    return [(reads[i], int(i)) for i in order]


def _world8_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    import json
    from gnnome_assembly_amd import dp, train as T
    dp.init_process_group("gloo")
    data = _mix24()
    sizes = [r for r, _ in data]
    mine = dp.shard_graphs(len(data), rank, world, sizes=sizes)
    tr = [mix_sample(*data[i]) for i in mine]
    va = [mix_sample(40, 100)] if rank == 0 else []
    first = {}

    def after_exchange(epoch, it, flat):
        if epoch == 0 and it == 0:
            first["grad"] = flat.grads.detach().numpy().copy()
            first["n"] = float(flat.contributors)
    hp = dict(num_epochs=2, dim_latent=32, num_gnn_layers=1, lr=1e-3, seed=0)
    workdir = os.path.join(out_dir, f"rank{rank}")
    os.makedirs(workdir, exist_ok=True)
    model, best, hist = T.train(tr, va, out="w8", hyperparameters=hp, workdir=workdir, verbose=False,
                                hooks={"after_exchange": after_exchange, "model_factory": oracle_model_factory,
                                       "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))})
    flat_order = sorted(model.parameters(), key=lambda p: p._gnm_slot)
    np.savez(os.path.join(out_dir, f"w8_{rank}.npz"), grad0=first["grad"],
             final=torch.cat([p.detach().reshape(-1) for p in flat_order]).numpy())
    json.dump({"shard": mine, "step_graph": hist.step_graph, "n0": first["n"], "loss_train": hist.loss_train,
               "loss_valid": hist.loss_valid, "lr": hist.lr, "tfpn_train": hist.tfpn_train,
               "files": sorted(os.path.relpath(os.path.join(d, f), workdir) for d, _, fs in os.walk(workdir) for f in fs)},
              open(os.path.join(out_dir, f"w8_{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_train_loop_under_eight_ranks_on_the_mixed_chromosome_set(tmp_path):
    import json
    world = 8
    mp.spawn(_world8_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    meta = [json.load(open(tmp_path / f"w8_{r}.json")) for r in range(world)]
    arrs = [np.load(tmp_path / f"w8_{r}.npz") for r in range(world)]
    data = _mix24()
    sizes = np.array([r for r, _ in data], dtype=np.float64)
    # every graph is trained on exactly once per epoch, three steps per rank and epoch, the ranks' steps stay aligned
    assert sorted(i for m in meta for i in m["shard"]) == list(range(24))
    assert all(len(m["step_graph"]) == 6 for m in meta)
    for ep in range(2):
        seen = sorted(m["shard"][k] for m in meta for k in m["step_graph"][3 * ep:3 * ep + 3])
        assert seen == list(range(24))
    # the per-rank idle fraction the sharding test predicts (step time ~ the step's largest graph): < 10 % in any step, < 5 %
    # of the epoch -- measured on what train.train actually ran (its own per-epoch shuffle of every rank's shard included)
    per_step = np.array([[sizes[meta[r]["shard"][meta[r]["step_graph"][k]]] for r in range(world)] for k in range(6)])
    worst = float((1.0 - per_step / per_step.max(1, keepdims=True)).max())
    epoch_idle = float((1.0 - per_step.sum(0) / per_step.max(1).sum()).max())
    print(f"eight ranks, 24 graphs: worst idle fraction of a rank in a step {worst:.3f}, over the run {epoch_idle:.3f}")
    assert worst < 0.10 and epoch_idle < 0.05
    # replicas stay bit-equal; epoch statistics agree on every rank; all eight contributed to the first exchange
    assert all(np.array_equal(arrs[0]["final"], a["final"]) for a in arrs[1:])
    assert all(np.array_equal(arrs[0]["grad0"], a["grad0"]) for a in arrs[1:])
    assert all(m["n0"] == 8.0 for m in meta)
    for key in ("loss_train", "loss_valid", "lr", "tfpn_train"):
        assert all(m[key] == meta[0][key] for m in meta[1:]), key
    # files come from rank 0 only
    assert "checkpoints/w8.pt" in meta[0]["files"] and all(not m["files"] for m in meta[1:])
    # the first exchanged gradient is the MEAN of the eight first-step graphs' single-graph gradients (fresh model, seed 0)
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import models, train as T
    torch.manual_seed(0)
    ref = oracle_model_factory(dict(T.get_hyperparameters(), dim_latent=32, num_gnn_layers=1))
    models.flatten_parameters(ref)
    order = sorted(ref.parameters(), key=lambda p: p._gnm_slot)
    ratios, samples = [], []
    for r in range(world):
        ss = [mix_sample(*data[i]) for i in meta[r]["shard"]]
        ratios.append((float(np.mean([float((s.y == 1).sum() / (s.y == 0).sum()) for s in ss])), len(ss)))
        samples.append(ss[meta[r]["step_graph"][0]])
    ratio = sum(a * n for a, n in ratios) / sum(n for _, n in ratios)
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([1.0 / ratio]))
    want = torch.zeros(sum(p.numel() for p in order))
    for s in samples:
        ref.zero_grad(set_to_none=True)
        crit(ref(s.graph, None, s.e, s.pe).squeeze(-1), s.y).backward()
        want += torch.cat([p.grad.reshape(-1) for p in order]) / world
    got = arrs[0]["grad0"]
    assert np.abs(got - want.numpy()).max() <= 2e-6 * max(1.0, float(want.abs().max()))
