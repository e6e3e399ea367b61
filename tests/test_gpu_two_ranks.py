"""Two (and four) real ranks -- separate processes, torch.distributed rendezvous, one HIP context each -- sharing the one
GPU of the test box.  RCCL refuses two ranks on one device, so the communicator's transport is the CALLBACK one (zkhip_comm_create:
an all-gather over gloo that stages the tiny payloads through host memory); everything else is the production path: the protocols
inside libzkhip (zkhip_sc_prove_sharded / zkhip_mc_prove_sharded / zkhip_gkr_prove_sharded / zkhip_kzg_commit_sharded), compared on
every rank with the single-GPU provers."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zk_cryptography_amd as zk
        from zk_cryptography_amd import _native as N
        from zk_cryptography_amd import distributed as D
        torch.cuda.set_device(0)
        shim = dist                     # gloo: distributed.Comm picks the staged (callback) transport

        def cuda(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()

        res = {}
        # basic sumcheck, stage form: 2^20 entries over `world` ranks
        full = zk.Fr.random(1 << 20, 4242)
        s, rp, ch = D.ShardedSumcheck(D.HipSumcheckEngine(cuda(D.shard_interleaved(full, rank, world))), world, None, shim).prove()
        sc = zk.Sumcheck(zk.Multilinear(full))
        sc.poly_sum()
        proof, wch = sc.prove()
        res["sumcheck"] = bool(np.array_equal(s, proof.sum) and np.array_equal(rp, proof.univariate_poly) and np.array_equal(ch, wch))
        # ComposedSumcheck::prove, three tables of 2^16
        tabs = [zk.Fr.random(1 << 16, 100 + k) for k in range(3)]
        eng = D.HipComposedEngine([[cuda(D.shard_interleaved(t, rank, world)) for t in tabs]], world, multi=False)
        rp, ch = D.ShardedComposedSumcheck(eng, world, None, shim).prove()
        wproof, wch = zk.ComposedSumcheck(zk.ComposedMultilinear([zk.Multilinear(t) for t in tabs])).prove()
        res["composed"] = bool(np.array_equal(rp, wproof.round_polys) and np.array_equal(ch, wch))
        # MultiComposedSumcheckProver::prove_partial, the GKR shape
        tabs = [zk.Fr.random(1 << 14, 200 + k) for k in range(4)]
        poly = [zk.ComposedMultilinear([zk.Multilinear(tabs[0]), zk.Multilinear(tabs[1])]),
                zk.ComposedMultilinear([zk.Multilinear(tabs[2]), zk.Multilinear(tabs[3])])]
        claimed = zk.MultiComposedSumcheckProver.calculate_poly_sum(poly)
        sh = [cuda(D.shard_interleaved(t, rank, world)) for t in tabs]
        eng = D.HipComposedEngine([sh[:2], sh[2:]], world, multi=True, claimed_sum=claimed)
        rps, ch = D.ShardedComposedSumcheck(eng, world, None, shim).prove()
        wproof, wch = zk.MultiComposedSumcheckProver.prove_partial(poly, claimed)
        got = [zk.SparseUnivariatePolynomial(c, p).monomials() for c, p in rps]
        res["multi_composed"] = bool(got == [p.monomials() for p in wproof.round_polys] and np.array_equal(ch, wch))
        # GKRProtocol::prove with every layer's sumcheck sharded (narrow layers run whole on every rank)
        def sharded_is_the_single_gpu_proof(circuit, inp):
            ev = circuit.evaluation(inp)
            want = zk.GKRProtocol.prove(circuit, ev)
            got = zk.GKRProtocol.prove_sharded(circuit, ev, world, rank, None, shim)
            ok = len(got.sumcheck_proofs) == len(want.sumcheck_proofs) and got._exchanges > 0
            for a, b in zip(got.sumcheck_proofs, want.sumcheck_proofs):
                ok = ok and np.array_equal(a.sum, b.sum) and a.to_bytes() == b.to_bytes()
            ok = ok and all(np.array_equal(a, b) for a, b in zip(got.wb_s, want.wb_s)) and all(np.array_equal(a, b) for a, b in zip(got.wc_s, want.wc_s))
            ok = ok and all(np.array_equal(a, b) for a, b in zip(got._challenges, want._challenges))
            return bool(ok), got

        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from gkr_cases import scrambled_circuit
        # scrambled wiring: CSR rows of uneven length, inputs shared between gates, b == c, every rank owns live rows of both phases
        # (Circuit::random's rows hold at most one gate, all of them on rank 0 in the rounds over b).  12: the widest layer whose eq tables are
        # still chains over the index bits; 14: gate weights (13 bits) and eq(u) (13, 14 bits) built from halves on the sharded path
        for depth, seed in ((9, 31), (12, 32), (14, 33)):
            ok, _ = sharded_is_the_single_gpu_proof(zk.Circuit.from_tuples(scrambled_circuit(depth, seed)), zk.Fr.random(2 ** depth, 500 + depth))
            res["gkr_scrambled_depth_%d" % depth] = ok
        for depth in (5, 9, 20):      # 20 = BASELINE configs[3]'s width (2^20-value layers)
            ok, got = sharded_is_the_single_gpu_proof(zk.Circuit.random(depth), zk.Fr.random(2 ** depth, 300 + depth))
            res["gkr_depth_%d" % depth] = ok
            if depth < 20 or rank == 0:   # and against the CPU oracle's sparse-container restatement of the reference prover (15 s at depth 20)
                from gkr_cases import gkr_proof_mismatches, random_circuit
                from oracle import oracle as ora
                layers = random_circuit(depth)
                o_ev = ora.circuit_evaluation(layers, zk.Fr.random(2 ** depth, 300 + depth))
                res["gkr_depth_%d_vs_oracle" % depth] = gkr_proof_mismatches(ora, got, ora.gkr_prove_sparse(layers, o_ev)) == []
        # sharded KZG commit
        tau = zk.Fr.random(12, 7)
        srs = zk.TrustedSetup.setup(tau)
        scal = zk.Fr.random(1 << 12, 8)
        want = zk.MultilinearKZG.commitment(zk.Multilinear(scal), srs)
        my_srs = zk.TrustedSetup(srs.powers_of_tau_in_g1[rank::world].contiguous(), srs.inf[rank::world].contiguous())
        my_poly = zk.Multilinear(cuda(D.shard_interleaved(scal, rank, world)))
        comm = D.Comm.get(N.Context.get(0), world, rank, dist, None)
        xy, inf = D.sharded_commit(my_srs.powers_of_tau_in_g1, my_srs.inf, my_poly.evaluations, comm)
        ok = (not inf) and np.array_equal(xy, want.xy)
        xy, inf = D.sharded_commit(None, my_srs.inf, my_poly.evaluations, comm, table=my_srs.precompute().table)   # the shard's shifted-SRS table
        ok = ok and (not inf) and np.array_equal(xy, want.xy)
        res["commit"] = bool(ok)
        res["exchanges_counted"] = comm.stats()[0] > 10
        D.Comm.close_all()
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_real_ranks_sharing_one_gpu(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=400) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, r in sorted(res):
        assert all(r.values()), (rank, [k for k, v in r.items() if not v])
    assert len(res) == world


def _worker_rccl_pick(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zk_cryptography_amd as zk
        from zk_cryptography_amd import _native as N
        from zk_cryptography_amd import distributed as D
        torch.cuda.set_device(0)
        D.Comm._pick_rccl_anyway = True          # what a job on the nccl backend picks: the library's own RCCL communicator
        comm = D.Comm.get(N.Context.get(0), world, rank, dist, None)
        full = zk.Fr.random(1 << 16, 777)
        t = torch.from_numpy(np.ascontiguousarray(D.shard_interleaved(full, rank, world)).view(np.int64)).cuda()
        s, rp, ch = D.ShardedSumcheck(D.HipSumcheckEngine(t), world, None, dist, comm=comm).prove()
        sc = zk.Sumcheck(zk.Multilinear(full))
        sc.poly_sum()
        proof, wch = sc.prove()
        ok = bool(np.array_equal(s, proof.sum) and np.array_equal(rp, proof.univariate_poly) and np.array_equal(ch, wch))
        q.put((rank, {"proof": ok, "transport": comm.transport, "fallback_reason": comm.fallback_reason}))
        D.Comm.close_all()
    finally:
        dist.destroy_process_group()


def test_rccl_communicator_that_does_not_come_up_falls_back_on_every_rank():
    """Two ranks on ONE device: the library's RCCL communicator cannot be built (RCCL refuses duplicate devices) or, if a build of RCCL
    allows it, works.  Either way every rank ends with the SAME transport -- the ranks agree over torch.distributed after a probe
    all-gather -- and the sharded proof is the single-GPU proof."""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker_rccl_pick, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    transports = {r["transport"] for _, r in res}
    assert len(transports) == 1 and transports <= {"rccl", "staged"}, res
    for _, r in res:
        assert r["proof"], res
        assert (r["transport"] == "staged") == (r["fallback_reason"] is not None), res


def _worker_nccl_like(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zk_cryptography_amd as zk
        from zk_cryptography_amd import _native as N
        from zk_cryptography_amd import distributed as D
        torch.cuda.set_device(0)

        class NcclLike:
            """What distributed.Comm sees of a job on the nccl backend: get_backend() says "nccl" and every tensor collective REFUSES CPU
            tensors the way ProcessGroupNCCL does.  (Underneath the bytes travel over gloo: two ranks share this box's one GPU.)"""
            ReduceOp = dist.ReduceOp
            cuda_collectives = 0

            def get_backend(self, group=None):
                return "nccl"

            def get_rank(self, group=None):
                return dist.get_rank(group)

            def get_global_rank(self, group, r):
                return dist.get_global_rank(group, r)

            def broadcast_object_list(self, box, src=0, group=None):
                dist.broadcast_object_list(box, src=src, group=group)

            def _need_cuda(self, *ts):
                if not all(t.is_cuda for t in ts):
                    raise RuntimeError("No backend type associated with device type cpu")
                NcclLike.cuda_collectives += 1

            def all_reduce(self, t, op=None, group=None):
                self._need_cuda(t)
                c = t.cpu()
                dist.all_reduce(c, op=op, group=group)
                t.copy_(c)

            def all_gather_into_tensor(self, out, inp, group=None):
                self._need_cuda(out, inp)
                c = out.cpu()
                dist.all_gather_into_tensor(c, inp.cpu(), group=group)
                out.copy_(c)

        shim = NcclLike()
        ctx = N.Context.get(0)
        full = zk.Fr.random(1 << 16, 778)
        sc = zk.Sumcheck(zk.Multilinear(full))
        sc.poly_sum()
        proof, wch = sc.prove()
        res = {}
        # (1) what such a job does by itself: picks the library's RCCL communicator, probes it, agrees, falls back together if needed
        comm = D.Comm.get(ctx, world, rank, shim, None)
        res["picked"] = comm.transport
        res["picked_reason"] = comm.fallback_reason
        # (2) the staged transport itself on the nccl-like group, whatever (1) ended with
        staged = comm if comm.transport == "staged" else D.Comm(ctx, world, rank, shim, None, transport="staged")
        before = NcclLike.cuda_collectives
        t = torch.from_numpy(np.ascontiguousarray(D.shard_interleaved(full, rank, world)).view(np.int64)).cuda()
        s, rp, ch = D.ShardedSumcheck(D.HipSumcheckEngine(t), world, None, shim, comm=staged).prove()
        res["proof"] = bool(np.array_equal(s, proof.sum) and np.array_equal(rp, proof.univariate_poly) and np.array_equal(ch, wch))
        res["exchanges_on_cuda_tensors"] = NcclLike.cuda_collectives - before
        # a sharded commit through it as well (one exchange of 128-byte records)
        tau = zk.Fr.random(10, 17)
        srs = zk.TrustedSetup.setup(tau)
        scal = zk.Fr.random(1 << 10, 18)
        want = zk.MultilinearKZG.commitment(zk.Multilinear(scal), srs)
        xy, inf = D.sharded_commit(srs.powers_of_tau_in_g1[rank::world].contiguous(), srs.inf[rank::world].contiguous(),
                                   torch.from_numpy(np.ascontiguousarray(D.shard_interleaved(scal, rank, world)).view(np.int64)).cuda(), staged)
        res["commit"] = bool((not inf) and np.array_equal(xy, want.xy))
        # closing a context closes its communicators; a later Comm.get on a new context never hands out a dead one
        n_before = len(D.Comm._cache)
        ctx.destroy()
        res["comms_closed_with_context"] = (not staged.handle) and (not comm.handle) and len(D.Comm._cache) < max(n_before, 1)
        ctx2 = N.Context.get(0)
        res["fresh_context"] = ctx2 is not ctx and bool(ctx2.handle)
        q.put((rank, res))
        D.Comm.close_all()
    finally:
        dist.destroy_process_group()


def test_staged_transport_on_a_group_that_only_takes_cuda_tensors():
    """The transport of last resort must work where it is needed: on an nccl process group (no CPU backend).  A shim that reports the
    nccl backend and rejects CPU tensors in every collective stands in for it on this one-GPU box: the auto-picked communicator
    ends the same on both ranks, and the staged transport -- forced if RCCL happened to come up -- proves and commits bit-exactly
    while every exchange it made went through CUDA tensors."""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker_nccl_like, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert len({r["picked"] for _, r in res}) == 1, res
    for _, r in res:
        assert r["picked"] in ("rccl", "staged") and (r["picked"] == "staged") == (r["picked_reason"] is not None), res
        assert r["proof"] and r["commit"] and r["exchanges_on_cuda_tensors"] >= 2, res
        assert r["comms_closed_with_context"] and r["fresh_context"], res


def test_soak_four_processes_one_gpu_device_transcript_and_sharded_gkr():
    """tools/soak_ranks.py, short form: four processes share the GPU and prove the same circuit again and again -- the device-resident outer
    transcript (whose hasher reads another workgroup's round items from behind another L2: the agent-scope release of round 5) and the
    sharded prover; every proof of every repeat on every rank identical.  (The 50-repeat form is run per round: profiles/r06/NOTES.md.)"""
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "soak_ranks.py"), "4", "6", "9,14"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "ALL IDENTICAL" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
