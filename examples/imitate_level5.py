#!/usr/bin/env python3
"""The level5 student from the collector to the evaluation, everything on one GPU: collect -> fit -> evaluate.

    python examples/imitate_level5.py --envs 256 --steps 64 --epochs 2
    python examples/imitate_level5.py --envs 2048 --steps 100 --capacity 400000 --batch-size 1024 --dump data/level5

Mirrors apps/threatsense_runner/collect_and_save.py (step Level5DumbMultiObs, keep the armed wingmen's valid observations and the
behaviour tree's commands) and run_student.py / SupervisedImitationTrainer._train_ppo (Adam on loss_mae_direction with
kill_high_correlation on last_action), without the HDF5 files in between: the rows stay in an ImitationDataset in device memory.
The student then flies the agent of `level5_fusion` through evaluate_policy with the fused sphere encoder."""
import argparse, json, os, sys, time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")  # the exhaustive convolution search costs minutes per new batch shape

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256, help="level5_dumb envs the collector steps (seven wingmen each)")
    ap.add_argument("--steps", type=int, default=64, help="collector steps")
    ap.add_argument("--capacity", type=int, default=0, help="rows the ring holds (default: everything the collector can produce)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--pytorch-encoder", action="store_true", help="train the conv blocks through autograd instead of the HIP kernels")
    ap.add_argument("--eval-envs", type=int, default=64)
    ap.add_argument("--eval-episodes", type=int, default=64)
    ap.add_argument("--dump", metavar="DIR", help="also write the collected rows as part files in the reference collector's layout")
    args = ap.parse_args()
    import numpy as np
    import torch
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.imitation import ImitationDataset
    from dronechase_amd.monitor import evaluate_policy
    from dronechase_amd.student import FLIAStudent, StudentDriver, StudentTrainer

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    collector = BatchedEnv(default_config("level5_dumb", n_envs=args.envs), dev)
    rows_per_step = args.envs * int(collector.cfg.n_pursuers)
    data = ImitationDataset(args.capacity or rows_per_step * args.steps, dev, rows_per_step)
    collector.reset()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    data.collect(collector, args.steps)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    collector.close()
    print(json.dumps({"collected_rows": data.total(), "kept_in_ring": data.size(), "ring_GiB": round(data.buf.numel() / 2 ** 30, 2),
                      "collect_steps_per_s": round(args.steps / (t1 - t0), 1)}), flush=True)
    if args.dump:
        written = data.to_dump(args.dump)
        print(json.dumps({"dump": args.dump, "files": len(written.files), "rows": written.rows_written}), flush=True)

    student = FLIAStudent().to(dev)
    trainer = StudentTrainer(student, lr=args.lr, fused_encoder=not args.pytorch_encoder)
    rng = np.random.default_rng(42)
    for epoch in range(args.epochs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        losses = trainer.fit(data, epochs=1, batch_size=args.batch_size, rng=rng)
        mean = float(losses.mean())         # the epoch's one host read
        print(json.dumps({"epoch": epoch, "batches": int(losses.numel()), "loss_mean": round(mean, 5), "loss_last": round(float(losses[-1]), 5),
                          "rows_per_s": round(data.size() / (time.perf_counter() - t0), 1)}), flush=True)

    env = BatchedEnv(default_config("level5_fusion", n_envs=args.eval_envs, seed=1), dev)
    returns, lengths = evaluate_policy(StudentDriver(student, fused_encoder=True), env, n_eval_episodes=args.eval_episodes)
    print(json.dumps({"eval_episodes": int(len(returns)), "eval_rew_mean": round(float(returns.mean()), 4), "eval_rew_std": round(float(returns.std()), 4),
                      "eval_len_mean": round(float(lengths.mean()), 2)}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
