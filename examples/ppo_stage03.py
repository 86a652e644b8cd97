#!/usr/bin/env python3
"""stage03 + PPO with everything on the GPU (BASELINE.json config 5): env shard, rollout storage, policy, update.

    python examples/ppo_stage03.py --envs 65536 --iters 5
    python examples/ppo_stage03.py --envs 8192 --episode-stats --eval-episodes 200
    python examples/ppo_stage03.py --envs 8192 --features-dim 512 --net-arch 128,256,512 --fused-forward    # the reference's trained shape
    python examples/ppo_stage03.py --envs 8192 --iters 20 --save models/stage03.pt --checkpoint-every 4000000 --eval-every 4000000
    python examples/ppo_stage03.py --envs 8192 --iters 20 --resume models/stage03.pt --save models/stage03.pt    # continues bit for bit
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/ppo_stage03.py --envs 8192

One process per GPU; each rank owns `--envs` environments (RNG keyed on the global env index) and the gradient
all-reduce is the only collective.  Mirrors apps/threatengage_runner/stage03 (PPO + LidarInertialActionExtractor,
rl_frequency 15, dome 20) without stable-baselines3."""
import argparse, json, os, sys, time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")  # the exhaustive convolution search costs minutes per new batch shape

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=32768)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--task", default="stage03")
    ap.add_argument("--episode-stats", action="store_true", help="log ep_rew_mean, ep_len_mean, ... of the episodes that finished in each collect (rank-local)")
    ap.add_argument("--eval-episodes", type=int, default=0, help="after training: evaluate the policy over N episodes on a fresh env (rank 0)")
    ap.add_argument("--features-dim", type=int, default=256, help="width of the policy's trunk (the reference trains 512)")
    ap.add_argument("--net-arch", type=lambda s: tuple(int(w) for w in s.split(",")), default=(64, 64),
                    help="widths of the pi / vf heads' hidden layers, e.g. 128,256,512 (the reference's h[128, 256, 512] checkpoints)")
    ap.add_argument("--fused-forward", action="store_true", help="the rollout's policy forward as one HIP launch (PPOConfig.fused_forward)")
    ap.add_argument("--save", metavar="PATH", help="after training: write a full checkpoint (PPO.save) to PATH and the SB3-named policy next to it (.zip)")
    ap.add_argument("--resume", metavar="PATH", help="continue bit for bit from a checkpoint of the same --task and --envs (PPO.load); --iters more iterations")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="TIMESTEPS", help="a checkpoint every TIMESTEPS into the directory of --save (or ./models)")
    ap.add_argument("--eval-every", type=int, default=0, metavar="TIMESTEPS",
                    help="evaluate over --eval-episodes episodes (default 10) on a separate env every TIMESTEPS: evaluations.npz, best_model.zip, "
                         "stop after 3 evaluations without a new best (not before the 6th)")
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig

    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    # TE_PPO_BACKEND=gloo: rehearsal on a box with fewer GPUs than ranks (the ranks share devices round-robin, the gradient bucket crosses
    # through the host); the real thing is nccl (= RCCL), one rank per GPU
    backend = os.environ.get("TE_PPO_BACKEND", "nccl")
    local = local if backend == "nccl" else local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    if world > 1 and (args.save or args.resume or args.checkpoint_every or args.eval_every):
        ap.error("--save, --resume, --checkpoint-every and --eval-every are single-process: a full checkpoint holds one rank's env shard")
    env = BatchedEnv(default_config(args.task, n_envs=args.envs, env_index_base=rank * args.envs), dev)
    callback, callback_env = None, None
    if args.checkpoint_every > 0 or args.eval_every > 0:   # the reference's callbacklist, frequencies in timesteps; the checkpoint last
        from dronechase_amd.callbacks import CallbackList, CheckpointCallback, EvalCallback, StopTrainingOnNoModelImprovement
        models = os.path.dirname(os.path.abspath(args.save)) if args.save else "./models"
        cbs = []
        if args.eval_every > 0:
            callback_env = BatchedEnv(default_config(args.task, n_envs=min(args.envs, 1024), seed=1), dev)
            cbs.append(EvalCallback(callback_env, n_eval_episodes=args.eval_episodes or 10, eval_freq=args.eval_every, best_model_save_path=models,
                                    log_path=models, callback_after_eval=StopTrainingOnNoModelImprovement(max_no_improvement_evals=3, min_evals=5)))
        if args.checkpoint_every > 0:
            cbs.append(CheckpointCallback(save_freq=args.checkpoint_every, save_path=models))
        callback = CallbackList(cbs)
    if args.resume:   # the config and the policy's shape are the checkpoint's; a callback list takes up its saved state (same flags as the saved run's)
        ppo = PPO.load(args.resume, env, callback=callback)
    else:
        ppo = PPO(env, PPOConfig(n_steps=args.n_steps, batch_size=args.batch_size, n_epochs=args.epochs, episode_stats=args.episode_stats,
                                 features_dim=args.features_dim, net_arch=args.net_arch, fused_forward=args.fused_forward), seed=0)
    if rank == 0:
        print(f"rollout buffer {ppo.buf.bytes() / 2**30:.1f} GiB on {dev}; policy parameters {sum(p.numel() for p in ppo.policy.parameters())}", flush=True)
    if callback is not None:   # learn() consults the callbacks after every update(); one line per iteration, no collect / update split
        per_iter, clock = ppo.cfg.n_steps * args.envs, [time.perf_counter()]

        def line(log):
            torch.cuda.synchronize(); now = time.perf_counter()
            print(json.dumps({"iter": log["timesteps"] // per_iter - 1, "env_steps": per_iter, "train_env_steps_per_s": per_iter / (now - clock[0]),
                              **{k: round(v, 5) for k, v in log.items() if k != "timesteps"}}), flush=True)
            clock[0] = time.perf_counter()

        target = ppo.num_timesteps + args.iters * per_iter
        ppo.learn(target, log=line, callback=callback)
        if ppo.num_timesteps < target:
            print(json.dumps({"stopped_at_timesteps": ppo.num_timesteps, "best_mean_reward": cbs[0].best_mean_reward}), flush=True)
    for it in range(args.iters if callback is None else 0):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = ppo.collect()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        u = ppo.update()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if rank == 0:
            n = ppo.cfg.n_steps * args.envs * world      # --resume: the checkpoint's n_steps, not --n-steps
            print(json.dumps({"iter": it, "env_steps": n, "collect_env_steps_per_s": n / (t1 - t0), "train_env_steps_per_s": n / (t2 - t0),
                              **{k: round(v, 5) for k, v in {**r, **u}.items()}}), flush=True)
    if world > 1:   # every rank applied the same mean gradient to the same initial weights: the replicas must still be identical
        flat = torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()]).double()
        lo, hi = flat.clone(), flat.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        if rank == 0:
            print(json.dumps({"world": world, "replicas_in_sync": bool(torch.equal(lo, hi)), "param_abs_sum": float(flat.abs().sum())}), flush=True)
    if args.eval_episodes > 0 and rank == 0:   # SB3's EvalCallback: a separate env, deterministic actions, raw rewards
        from dronechase_amd.pipeline import ReinforcementLearningPipeline
        eval_env = BatchedEnv(default_config(args.task, n_envs=min(args.envs, 1024), seed=1), dev)
        avg, std, n, _ = ReinforcementLearningPipeline.evaluate(ppo, eval_env, n_eval_episodes=args.eval_episodes)
        print(json.dumps({"eval_episodes": n, "eval_rew_mean": avg, "eval_rew_std": std}), flush=True)
        eval_env.close()
    if args.save:
        ppo.save(args.save)
        ppo.save_policy(os.path.splitext(args.save)[0] + ".zip")
        print(json.dumps({"saved": args.save, "bytes": os.path.getsize(args.save), "timesteps": ppo.num_timesteps}), flush=True)
    if callback_env is not None:   # after save(): the checkpoint holds the evaluation env's state too
        callback_env.close()
    env.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
