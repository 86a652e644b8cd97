#!/usr/bin/env python3
"""What a checkpoint costs at the size people train at (profiles/ppo_checkpoint.json; DESIGN.md 7, callbacks.CheckpointCallback):
stage03 x 65 536 envs, the reference's BO shape (features_dim 512, net_arch (128, 256, 512)), n_steps 32, every fused switch on.

    python tools/ppo_checkpoint_bench.py --out profiles/ppo_checkpoint.json

In one process: two warm-up iterations, then `--repeats` times one learn() iteration with no checkpoint (wall time between two device
synchronisations) followed by one PPO.save() into a temporary directory (wall time of the call: it ends with the file written) and
one PPO.load() of that file into a second env of the same config.  Reported: median, min and max of each, the file's size, and the
ratio of the median save to the median iteration."""
import argparse, json, os, statistics, sys, tempfile, time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "repeats": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=32768)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the checkpoint is written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig

    dev = torch.device("cuda", 0)
    cfg = PPOConfig(n_steps=args.n_steps, batch_size=args.batch_size, n_epochs=args.epochs, features_dim=512, net_arch=(128, 256, 512),
                    fused_forward=True, fused_forward_bf16=True, fused_update=True, fused_update_wide=True, fused_update_bf16=True,
                    fused_optimizer=True, fused_advantages=True, fused_epoch=True, episode_stats=True)
    env = BatchedEnv(default_config("stage03", n_envs=args.envs), dev)
    ppo = PPO(env, cfg, seed=0)
    per_iter = args.n_steps * args.envs
    ppo.learn(2 * per_iter)
    iters, saves, loads, size = [], [], [], 0
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, "ckpt.pt")
        for _ in range(args.repeats):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ppo.learn(ppo.num_timesteps + per_iter)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            ppo.save(path)
            t2 = time.perf_counter()
            iters.append(t1 - t0); saves.append(t2 - t1)
            size = os.path.getsize(path)
        other = BatchedEnv(default_config("stage03", n_envs=args.envs), dev)
        for _ in range(min(args.repeats, 3)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            PPO.load(path, other)
            torch.cuda.synchronize(); loads.append(time.perf_counter() - t0)
        other.close()
    out = {"device": torch.cuda.get_device_name(0), "command": "python tools/ppo_checkpoint_bench.py " + " ".join(sys.argv[1:]),
           "task": "stage03", "n_envs": args.envs, "n_steps": args.n_steps, "batch_size": args.batch_size, "n_epochs": args.epochs,
           "features_dim": 512, "net_arch": [128, 256, 512], "timesteps_per_iteration": per_iter,
           "learn_iteration": spread(iters), "save": spread(saves), "load": spread(loads), "file_bytes": size,
           "env_state_bytes": env.state_words() * 4,
           "save_over_iteration": statistics.median(saves) / statistics.median(iters)}
    env.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
