"""RL pipelines with the reference's class names, constructor arguments and method surface
(pipeline/base.py:27-136 ReinL, pipeline/mat_invent.py:17-290 MatInvent, pipeline/baseline.py Baseline).
Sampling and fine-tuning run on the HIP path; scoring and filtering are the caller's plug-ins (rewards / filters are out of scope and
optional here); sample_cfg.mlip_opt, a callable (strucs, xyz_path) -> (strucs, energies) such as relax.Relaxer, relaxes the
valid samples before the filter and the reward see them, where the reference does; the long-term memory and its diversity filter are
memory.LongTimeMem, by formula as in the reference or by structure
(DESIGN 32)."""
import logging
import os
import time

import numpy as np
import torch

from . import config as C
from .dist import broadcast_object, rank_world
from .filters import invalid_filter
from .finetune import ft_step as _ft_step
from .memory import LongTimeMem, ReplayBuffer
from .structure import write_extxyz
from .suite import get_device


class ReinL:
    def __init__(self, rl_epoch, model_suite, reward, sample_cfg, finetune_cfg, save_dir, save_freq, device=None, logger=None,
                 replay=False, replay_args=None, **kwargs):
        self.rl_epoch, self.model_suite, self.reward = rl_epoch, model_suite, reward
        self.save_dir, self.save_freq, self.logger = save_dir, save_freq, logger
        self.device = get_device(device)
        self.cfg = C.create(kwargs)
        self.step, self.cost = 0, 0
        self.sample_cfg = C.merge(model_suite.sample_cfg, sample_cfg)          # pipeline wins (base.py:53-59)
        self.finetune_cfg = C.merge(model_suite.finetune_cfg, finetune_cfg)
        from .suite import MatterGenSuite
        if isinstance(model_suite, MatterGenSuite) and self.sample_cfg.get("sample_steps") is not None:
            raise ValueError("sample_cfg.sample_steps is the DiffCSP suite's strided reverse chain; the MatterGen suite has `sampling_steps` "
                             "of its own")
        self.sampler = model_suite.get_sampler()
        self.smact = None   # sample_cfg.smact: a path or {table, use_pauling_test, include_alloys, max_combos}; built once, its table on first use
        if self.sample_cfg.get("smact") is not None:
            from .chemistry import make_smact
            self.smact = make_smact(self.sample_cfg.get("smact"))
        self.models_dir = os.path.join(save_dir, "models")
        self.sample_dir = os.path.join(save_dir, "samples")
        os.makedirs(self.models_dir, exist_ok=True)
        os.makedirs(self.sample_dir, exist_ok=True)
        self.replay = ReplayBuffer(**(replay_args or {})) if replay else None
        self.ltm = LongTimeMem()   # base.py:64

    def relax_step(self, strucs, xyz_path=None):
        """mat_invent.py:88-91: sample_cfg.mlip_opt(strucs, xyz_path) -> (relaxed structures, energies), or (strucs, None, {}) without the
        key.  `data` -- what the fine-tune set is drawn from -- is never relaxed, as in the reference.  The third value: the log keys
        relax_converged, relax_failed, relax_steps_mean, relax_de_mean."""
        opt = self.sample_cfg.get("mlip_opt")
        if opt is None:
            return strucs, None, {}
        if not callable(opt):
            raise ValueError(f"sample_cfg.mlip_opt takes a callable (strucs, xyz_path) -> (strucs, energies), e.g. relax.Relaxer, not {type(opt).__name__}")
        from .relax import log_metrics
        relaxed, energies = opt(strucs, xyz_path)
        if len(relaxed) != len(strucs) or len(energies) != len(strucs):
            raise ValueError(f"sample_cfg.mlip_opt returned {len(relaxed)} structures and {len(energies)} energies for {len(strucs)} samples")
        log = log_metrics(opt, energies)
        logging.info("relaxation: " + ", ".join(f"{k}: {v}" for k, v in log.items()))
        return list(relaxed), energies, log

    def reward_step(self, sample_data, sample_struc, xyz_path=None, label="tmp"):
        """base.py:98-127: score, drop failed samples."""
        rewards, prop_dict, failed = self.reward.scoring((sample_struc, xyz_path), label)
        self.cost += len(sample_struc)
        ok = ~np.asarray(failed)
        data = [d for d, k in zip(sample_data, ok) if k]
        strucs = [s for s, k in zip(sample_struc, ok) if k]
        return data, strucs, np.asarray(rewards)[ok].astype(float), {k: np.asarray(v)[ok] for k, v in prop_dict.items()}

    def _smact_log(self):
        """{"smact_valid_frac": the share of the latest sampled batch whose composition passed}, or {} without sample_cfg.smact."""
        if self.smact is None:
            return {}
        last = self.smact.last
        return {"smact_valid_frac": float(last.valid.mean()) if last is not None and len(last) else float("nan")}


class MatInvent(ReinL):
    def __init__(self, rl_epoch, model_suite, reward, sample_cfg, finetune_cfg, topk_ratio, save_dir, save_freq=50, device=None,
                 logger=None, replay=False, replay_args=None, div_filter=False, df_args=None, **kwargs):
        super().__init__(rl_epoch=rl_epoch, model_suite=model_suite, reward=reward, sample_cfg=sample_cfg, finetune_cfg=finetune_cfg,
                         save_dir=save_dir, save_freq=save_freq, device=device, logger=logger, replay=replay, replay_args=replay_args,
                         **kwargs)
        assert 0.0 < topk_ratio <= 1.0
        self.topk_ratio = topk_ratio
        self.div_filter = bool(div_filter)
        self.df_args = dict(df_args or {})   # tol, buff, method ("composition" | "element_comb" | "structure"), fp_tol: LongTimeMem.div_filter's
        fp_args = self.df_args.pop("fp_args", None)   # r_max / nbins / sigma of the fingerprint, for the memory's clustering
        by_structure = self.replay is not None and self.replay.key == "structure"
        if self.df_args.get("method") == "structure" or by_structure:   # the memory clusters its rows by fingerprint as they come in (rank 0)
            fp_tol = self.df_args.get("fp_tol", self.replay.fp_tol if by_structure else None)
            self.ltm = LongTimeMem(structure=True, fp_args=dict(fp_args or (self.replay.fp_args if by_structure else {})),
                                   **({} if fp_tol is None else {"fp_tol": fp_tol}))
        self.load_model()

    def load_model(self):
        """mat_invent.py:62-72: agent (trainable) + frozen prior, two separate loads."""
        self.agent = self.model_suite.load_model()
        self.prior = self.model_suite.load_model()
        from .guidance import refuse_latent
        refuse_latent((self.agent, self.prior), type(self).__name__)   # (before any device work of the run: RL on a conditional prior is not built)
        for p in self.agent.parameters():
            p.requires_grad = True
        for p in self.prior.parameters():
            p.requires_grad = False
        self.agent.to(self.device)
        self.prior.to(self.device)

    def sample_step(self):
        """mat_invent.py:74-123: sample, geometric validity pre-filter (device-side quantities), save the valid set as
        extxyz, the optional relaxation (sample_cfg.mlip_opt: relax_step), the optional filter callable -- which receives the
        relaxation's energies, None without one --, max_num.  The stability metric of SUN is stability.SUNFilter, which reads those
        energies; the synthesizability metric is out of scope.
        sample_cfg.target_compositions_dict (a list of {symbol: count}) reaches the sampler with the other keys: the loop then samples
        crystals of those formulas only (replacement conditioning) and fine-tunes on them -- a fixed-formula RL loop.
        sample_cfg.resample_times / sample_cfg.jump_length reach it the same way: the conditioned chains make RePaint's jumps.
        sample_cfg.symmetry_template / sample_cfg.symmetry_fix_types too: every crystal is sampled under the template's space group.
        sample_cfg.smact never reaches the sampler: its mask is ANDed into the pre-filter and smact_valid_frac is logged."""
        rank, world = rank_world()
        kw = {k: v for k, v in self.sample_cfg.items() if k not in ("filter", "mlip_opt", "geometric_filter", "smact")}
        if self.sample_steps is not None:   # (the sampler builds the agent's strided view; ft_step stays on the agent and its trained grid)
            logging.info(f"sampling on {self.sample_steps} of the model's {self.agent.beta_scheduler.timesteps} steps")
        data, strucs = self.sampler.generate(model=self.agent, rank=rank, world_size=world, **kw)
        if self.sample_cfg.get("geometric_filter", True):  # the reference always filters (mat_invent.py:78-79)
            n_all = len(data)
            data, strucs = invalid_filter(data, strucs, **({} if self.smact is None else {"smact": self.smact}))
            logging.info(f"geometric pre-filter kept {len(data)} of {n_all} samples")
        elif self.smact is not None:
            keep = self.smact(data)
            data, strucs = [d for d, k in zip(data, keep) if k], [s for s, k in zip(strucs, keep) if k]
        xyz = None
        if rank == 0 and getattr(self, "sample_dir", None):
            xyz = write_extxyz(strucs, os.path.join(self.sample_dir, f"step_{self.step:0>4d}_valid.extxyz"))
        strucs, energies, relax_log = self.relax_step(strucs, xyz)
        flt = self.sample_cfg.get("filter")
        metrics = {}
        if callable(flt):
            data, strucs, metrics = flt(data, strucs, energies)
        metrics = dict(metrics, **relax_log, **self._smact_log())
        max_num = self.sample_cfg.get("max_num")
        if max_num and len(strucs) > max_num:
            data, strucs = data[:max_num], strucs[:max_num]
        return data, strucs, None, metrics

    @property
    def sample_steps(self):
        """sample_cfg.sample_steps: the reverse chain runs on that many of the model's trained steps (DiffCSPModule.respaced).
        Absent or null: all of them, nothing re-spaced."""
        s = self.sample_cfg.get("sample_steps")
        return None if s is None else int(s)

    def ft_step(self, data_list, rewards, baseline=None):
        return _ft_step(self.agent, self.prior, data_list, rewards, self.finetune_cfg, device=self.device)

    def _score_and_remember(self, data, strucs, xyz, metrics, log_now=True):
        """Rank 0's bookkeeping between sampling and the update: reward_step, the long-term memory with its five log keys, the logger's row
        (log_now=False: the caller adds its own keys and logs), then the diversity filter (mat_invent.py:230-237).  Returns (data, strucs,
        rewards -- penalised when the filter is on --, the log dict, the structures the filter zeroed)."""
        data, strucs, rewards, props = self.reward_step(data, strucs, xyz, f"step_{self.step:0>4d}")
        log = {f"{k} mean": v.mean() for k, v in props.items()}
        log.update({"reward mean": rewards.mean(), "reward std": rewards.std(), "cost": self.cost}, **metrics)
        # long-term memory (mat_invent.py:209-226): bookkeeping and five log keys, whether or not the filter is on
        self.ltm.extend(strucs, rewards, self.step)
        thred = getattr(self.reward, "threshold", getattr(self.reward, "reward_threshold", 0.0))
        burden, div_ratio = self.ltm.calc_metrics(thred)
        self.ltm.save(os.path.join(self.sample_dir, "long_term_memory.csv"))
        logging.info(f"{len(self.ltm)} crystals generated so far, {len(self.ltm.unique_comps)} unique components.  Burden: {burden}, "
                     f"Div. Ratio: {div_ratio}.")
        log.update({"crystal_num": len(self.ltm), "unique_comps": len(self.ltm.unique_comps), "burden": burden, "div_ratio": div_ratio})
        if self.ltm.structure:
            log["unique_structures"] = self.ltm.unique_structures
        if log_now and self.logger is not None:
            self.logger.log(log, step=self.step)
        penalty_strucs = []
        if self.div_filter:   # (mat_invent.py:230-237: the penalised rewards rank the top-k)
            rewards, penalty_idx, tol_n, buff_n = self.ltm.div_filter(strucs, rewards, **self.df_args)
            penalty_strucs = [strucs[p] for p in penalty_idx]
            logging.info(f"Diversity filter: tol_n={tol_n}, buff_n={buff_n}")
        return data, strucs, rewards, log, penalty_strucs

    def rl_step(self):
        t0 = time.time()
        rank, world = rank_world()
        logging.info(f"*****   LOOP {self.step} START   *****")
        data, strucs, xyz, metrics = self.sample_step()
        if len(data) == 0:  # (the reference would fail inside reward scoring; identical on every rank, so no rank diverges)
            logging.warning("no sample passed the validity pre-filter; skipping scoring and fine-tuning for this loop")
            return
        if rank == 0:  # scoring / ranking / replay are rank-0 CPU bookkeeping; the chosen set is broadcast
            data, strucs, rewards, _, penalty_strucs = self._score_and_remember(data, strucs, xyz, metrics)
            order = np.argsort(rewards)[::-1]
            topk = order[: int(self.finetune_cfg.batch_size * self.topk_ratio)]
            ft_data, ft_reward = [data[i] for i in topk], rewards[topk]
            if self.replay is not None:
                if penalty_strucs:
                    self.replay.memory_purge(penalty_strucs)
                rd, rr = self.replay.sample()
                self.replay.extend(ft_data, None, ft_reward)
                ft_data, ft_reward = ft_data + rd, np.concatenate((ft_reward, rr))
            payload = (ft_data, ft_reward)
        else:
            payload = None
        ft_data, ft_reward = broadcast_object(payload, src=0)
        self.ft_step(ft_data, ft_reward)
        logging.info(f"*****   LOOP {self.step} FINISH   *****  {(time.time() - t0) / 60:.2f} min")

    def run_rl(self):
        rank, _ = rank_world()
        for step in range(self.rl_epoch):
            self.step = step
            self.rl_step()
            if (step + 1) % self.save_freq == 0 and rank == 0:
                self.model_suite.save_model(self.agent, os.path.join(self.models_dir, f"loop_{step:0>4d}"))
        if rank == 0:
            self.model_suite.save_model(self.agent, os.path.join(self.models_dir, "final"))


class Baseline(ReinL):
    """pipeline/baseline.py: sample + score only (no fine-tuning); with the reference's 2-of-3 unpack
    bug (:78) fixed.  sample_cfg.mlip_opt relaxes the samples before they are scored (relax_step)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.agent = self.model_suite.load_model().to(self.device)

    def rl_step(self):
        kw = {k: v for k, v in self.sample_cfg.items() if k not in ("filter", "mlip_opt", "geometric_filter", "smact")}
        data, strucs = self.sampler.generate(model=self.agent, **kw)
        if self.smact is not None:   # (the composition test alone; the baseline has no geometric pre-filter)
            keep = self.smact(data)
            data, strucs = [d for d, k in zip(data, keep) if k], [s for s, k in zip(strucs, keep) if k]
            if not data:
                logging.warning("no sample passed the composition test; nothing is scored in this loop")
                if self.logger is not None:
                    self.logger.log(self._smact_log(), step=self.step)
                return
        strucs, _, relax_log = self.relax_step(strucs)
        data, strucs, rewards, props = self.reward_step(data, strucs, None, f"step_{self.step:0>4d}")
        if self.logger is not None:
            self.logger.log(dict({"reward mean": rewards.mean(), "reward std": rewards.std()}, **relax_log, **self._smact_log()), step=self.step)

    def run_rl(self):
        for step in range(self.rl_epoch):
            self.step = step
            self.rl_step()


class MatInventPG(MatInvent):
    """MatInvent with the PPO-clipped policy gradient on recorded trajectories (policy.pg_step, DDPO-style) in place of the
    reward-weighted denoising loss.  Each RL loop: rollout (sampling.sample_rollout: the kept crystals' chains stay on the device) ->
    the validity pre-filter, the optional relaxation (sample_cfg.mlip_opt), the optional filter callable and max_num, as in MatInvent ->
    reward_step -> pg_step over EVERY kept
    crystal.  On-policy: there is no top-k and no replay (a stored crystal's log-probabilities belong to weights that no longer exist),
    so replay=True is refused.  Single GPU, DiffCSP only (MatterGen has no log-probability path), one sampling batch per loop.
    finetune_cfg.kl_coef > 0 anchors the agent's transitions to the frozen prior's (policy.pg_step) and logs prior_kl.
    sample_cfg.sample_steps = S: rollout and training run through strided views of agent and prior and `rollout steps` is logged.
    sample_cfg.target_compositions_dict / condition (conditioned sampling) are refused by default: the record of a conditioned
    chain is not its likelihood.  sample_cfg.condition_likelihood: free lifts the refusal: the condition is built as
    DiffCSPSampler.generate builds it (target_compositions_dict: batch_size crystals cycling through the list, every atom type fixed; or an
    explicit conditioning.Condition for batch_size crystals), the rollout records -- and pg_step re-evaluates -- the likelihood over the
    free elements, and the condition follows the kept crystals through the filters and max_num.
    sample_cfg.resample_times / jump_length (resampling jumps) are refused: a rollout holds one visit per level."""

    def __init__(self, rl_epoch, model_suite, reward, sample_cfg, finetune_cfg, save_dir, save_freq=50, device=None, logger=None,
                 replay=False, replay_args=None, topk_ratio=1.0, **kwargs):
        from .suite import MatterGenSuite
        if replay:
            raise ValueError("MatInventPG is on-policy: replay=True is not supported (replayed crystals carry log-probabilities of "
                             "earlier weights)")
        if isinstance(model_suite, MatterGenSuite):
            raise ValueError("MatInventPG needs the DiffCSP suite: the MatterGen suite has no trajectory log-probability path")
        if rank_world()[1] > 1:
            raise ValueError("MatInventPG runs on one GPU: world_size > 1 is not supported")
        merged = C.merge(model_suite.sample_cfg, sample_cfg)
        lik = merged.get("condition_likelihood")
        if lik not in (None, "free"):
            raise ValueError(f"MatInventPG: sample_cfg.condition_likelihood = {lik!r} is neither null nor 'free'")
        if lik is not None and merged.get("target_compositions_dict") is not None and merged.get("condition") is not None:
            raise ValueError("MatInventPG: give sample_cfg.target_compositions_dict or sample_cfg.condition, not both")
        for k in ("target_compositions_dict", "condition"):
            if merged.get(k) is not None and lik is None:
                raise ValueError(f"MatInventPG: sample_cfg.{k} is not supported -- a conditioned chain's recorded log-probabilities are those "
                                 "of the unconditioned proposal, not a trajectory likelihood (use pipeline=mat_invent)")
        from .resampling import refuse
        refuse("MatInventPG", **{f"sample_cfg.{k}": merged.get(k) for k in ("resample_times", "jump_length")})
        from .steering import refuse as refuse_steer
        refuse_steer("MatInventPG", **{"sample_cfg.steer": merged.get("steer")})   # 
        from .classifier import refuse as refuse_classifier
        refuse_classifier("MatInventPG", **{"sample_cfg.classifier": merged.get("classifier")})   # 
        from .symmetry_constraint import refuse as refuse_symmetry
        refuse_symmetry("MatInventPG", **{f"sample_cfg.{k}": merged.get(k) for k in ("symmetry_template", "symmetry_fix_types")})   # 
        if kwargs.get("div_filter"):
            raise ValueError("MatInventPG: div_filter=True is not built -- the diversity filter penalises the rewards that rank a top-k, and the "
                             "policy gradient has no top-k (use pipeline=mat_invent)")
        nb = merged.get("num_batches", 1)
        if int(nb or 1) != 1:
            raise ValueError(f"MatInventPG samples one batch per loop: num_batches = {nb} is not supported")
        super().__init__(rl_epoch=rl_epoch, model_suite=model_suite, reward=reward, sample_cfg=sample_cfg, finetune_cfg=finetune_cfg,
                         topk_ratio=topk_ratio, save_dir=save_dir, save_freq=save_freq, device=device, logger=logger, replay=False,
                         replay_args=None, **kwargs)

    def _condition_kwargs(self):
        """sample_rollout's condition / likelihood keywords from sample_cfg (condition_likelihood: free), or none."""
        lik = self.sample_cfg.get("condition_likelihood")
        targets, cond = self.sample_cfg.get("target_compositions_dict"), self.sample_cfg.get("condition")
        if targets is not None and len(targets) == 0:
            targets = None
        if lik is None or (targets is None and cond is None):
            return {}
        if targets is not None:   # as DiffCSPSampler.generate: the crystals cycle through the list, every atom type fixed
            from .conditioning import Condition
            cond = Condition.composition([dict(t) for t in targets], int(self.sample_cfg.batch_size))
        return dict(condition=cond, likelihood=lik)

    def sample_step(self):
        """Rollout + the MatInvent sample step's filtering.  Returns (data, strucs, rollout restricted to data, metrics)."""
        from .data import data2struc
        from .sampling import sample_rollout
        self.sampler.seed += 1
        data, rollout = sample_rollout(int(self.sample_cfg.batch_size), self.agent, seed=self.sampler.seed,
                                       geometric_filter=bool(self.sample_cfg.get("geometric_filter", True)), sample_steps=self.sample_steps,
                                       **self._condition_kwargs(), **({} if self.smact is None else {"smact": self.smact}))
        strucs = [data2struc(d) for d in data]
        logging.info(f"rollout kept {len(data)} samples" + (f" over {rollout.T} steps" if self.sample_steps is not None else ""))
        xyz = None
        if getattr(self, "sample_dir", None):
            xyz = write_extxyz(strucs, os.path.join(self.sample_dir, f"step_{self.step:0>4d}_valid.extxyz"))
        strucs, energies, relax_log = self.relax_step(strucs, xyz)
        pos = {id(d): i for i, d in enumerate(data)}
        flt = self.sample_cfg.get("filter")
        metrics = {}
        if callable(flt):
            data, strucs, metrics = flt(data, strucs, energies)
        metrics = dict(metrics, **relax_log, **self._smact_log())
        max_num = self.sample_cfg.get("max_num")
        if max_num and len(strucs) > max_num:
            data, strucs = data[:max_num], strucs[:max_num]
        self._rollout_pos = pos
        return data, strucs, rollout, metrics

    def rl_step(self):
        from .policy import pg_step
        t0 = time.time()
        logging.info(f"*****   LOOP {self.step} START   *****")
        data, strucs, rollout, metrics = self.sample_step()
        if len(data) == 0:
            logging.warning("no sample passed the validity pre-filter; skipping scoring and the policy-gradient update for this loop")
            return
        data, strucs, rewards, props = self.reward_step(data, strucs, None, f"step_{self.step:0>4d}")
        log = {f"{k} mean": v.mean() for k, v in props.items()}
        log.update({"reward mean": rewards.mean() if len(rewards) else float("nan"),
                    "reward std": rewards.std() if len(rewards) else float("nan"), "cost": self.cost}, **metrics)
        if len(data) < 2:
            logging.warning(f"{len(data)} scored sample(s): the advantages need at least two; skipping the policy-gradient update for "
                            "this loop")
            if self.logger is not None:
                self.logger.log(log, step=self.step)
            return
        rollout = rollout.select([self._rollout_pos[id(d)] for d in data])
        agent, prior = self.agent, self.prior
        if self.sample_steps is not None:   # the views the rollout was recorded through: same theta, the strided grid
            agent, prior = agent.respaced(self.sample_steps), prior.respaced(self.sample_steps)
            log["rollout steps"] = rollout.T
        stats = pg_step(agent, rollout, rewards, self.finetune_cfg, seed=self.sampler.seed, prior=prior)
        last = stats[-1] if stats else {}
        log.update({"clip_frac": last.get("clip_frac", float("nan")), "approx_kl": last.get("approx_kl", float("nan")),
                    "ratio mean": last.get("ratio_mean", float("nan"))})
        if float(self.finetune_cfg.get("kl_coef", 0.0) or 0.0) > 0.0:
            log["prior_kl"] = last.get("prior_kl", float("nan"))
        for k in ("grad_norm", "skipped_steps"):   # (finetune_cfg.max_grad_norm / skip_nonfinite_steps: the optimiser's statistics)
            if k in last:
                log[k] = last[k]
        if self.logger is not None:
            self.logger.log(log, step=self.step)
        logging.info(f"*****   LOOP {self.step} FINISH   *****  {(time.time() - t0) / 60:.2f} min")


class MatInventDPO(MatInvent):
    """MatInvent with the preference loss on ranked pairs of final crystals (preference.dpo_step, Diffusion-DPO) in place of the
    reward-weighted denoising loss.  sample_step, reward_step, the long-term memory and the diversity filter are MatInvent's; each loop's
    pool is its scored crystals (with the penalised rewards when div_filter is on) plus replay.sample() when replay=True, and the loop's
    crystals then go into the replay buffer.  Pairs: preference.build_pairs over the pool with finetune_cfg.dpo_margin (default 0),
    finetune_cfg.dpo_pairs (the cap; default finetune_cfg.batch_size), finetune_cfg.dpo_within (null | formula: both crystals of a pair
    share the reduced formula), winners among the top `topk_ratio` share of the pool by reward (1.0: any), seed = the loop index.  The loss
    needs no trajectory and no on-policy data: conditioned sampling, sample_steps, num_batches > 1, replay and div_filter are all allowed.
    One GPU, DiffCSP only.  finetune_cfg.dpo_beta is required (preference.dpo_step)."""

    def __init__(self, rl_epoch, model_suite, reward, sample_cfg, finetune_cfg, save_dir, topk_ratio=1.0, **kwargs):
        from .suite import MatterGenSuite
        if isinstance(model_suite, MatterGenSuite):
            raise ValueError("MatInventDPO needs the DiffCSP suite: the MatterGen-shaped module has no fused micro-step to put the "
                             "preference loss in")
        if rank_world()[1] > 1:
            raise ValueError("MatInventDPO runs on one GPU: world_size > 1 is not supported (pairs cross shards)")
        super().__init__(rl_epoch=rl_epoch, model_suite=model_suite, reward=reward, sample_cfg=sample_cfg, finetune_cfg=finetune_cfg,
                         topk_ratio=topk_ratio, save_dir=save_dir, **kwargs)
        within = self.finetune_cfg.get("dpo_within")
        if within not in (None, "formula"):
            raise ValueError(f"MatInventDPO: finetune_cfg.dpo_within = {within!r} is neither null nor 'formula'")

    def make_pairs(self, pool, rewards):
        """preference.build_pairs over the pool under finetune_cfg's dpo_* keys and topk_ratio (see the class)."""
        from .memory import _formula
        from .preference import build_pairs
        fc = self.finetune_cfg
        rewards = np.asarray(rewards, dtype=float)
        winners = None
        if self.topk_ratio < 1.0:
            winners = np.zeros(len(pool), dtype=bool)
            winners[np.argsort(-rewards, kind="stable")[: max(1, int(len(pool) * self.topk_ratio))]] = True
        cap = fc.get("dpo_pairs")
        return build_pairs(rewards, keys=[_formula(d) for d in pool] if fc.get("dpo_within") == "formula" else None,
                           margin=float(fc.get("dpo_margin") or 0.0), max_pairs=int(fc.batch_size if cap is None else cap), winners=winners,
                           seed=self.step)

    def rl_step(self):
        from .preference import dpo_step
        t0 = time.time()
        logging.info(f"*****   LOOP {self.step} START   *****")
        data, strucs, xyz, metrics = self.sample_step()
        if len(data) == 0:
            logging.warning("no sample passed the validity pre-filter; skipping scoring and the preference update for this loop")
            return
        data, strucs, rewards, log, penalty_strucs = self._score_and_remember(data, strucs, xyz, metrics, log_now=False)
        pool, pool_rewards = list(data), np.asarray(rewards, dtype=float)
        if self.replay is not None:
            if penalty_strucs:
                self.replay.memory_purge(penalty_strucs)
            rd, rr = self.replay.sample()
            self.replay.extend(data, None, rewards)
            pool, pool_rewards = pool + rd, np.concatenate((pool_rewards, rr))
        pairs = self.make_pairs(pool, pool_rewards)
        log["pairs"] = len(pairs)
        if len(pairs) == 0:
            logging.warning(f"no pair among {len(pool)} crystals passes the margin / key / winner rules; skipping the preference update for "
                            "this loop")
        else:
            last = dpo_step(self.agent, self.prior, pool, pairs, self.finetune_cfg, device=self.device)[-1]
            log.update({"dpo_loss": last["loss"], "pref_acc": last["pref_acc"], "margin": last["margin"]})
            for k in ("grad_norm", "skipped_steps"):   # (finetune_cfg.max_grad_norm / skip_nonfinite_steps: the optimiser's statistics)
                if k in last:
                    log[k] = last[k]
        if self.logger is not None:
            self.logger.log(log, step=self.step)
        logging.info(f"*****   LOOP {self.step} FINISH   *****  {(time.time() - t0) / 60:.2f} min")


class Pretrain:
    """Supervised denoising training of a DiffCSP prior on a crystal dataset (pretrain.fit): the pipeline that produces the
    model the RL pipelines start from.  train_path / val_path: extxyz files (structure.read_extxyz); train_cfg: pretrain.fit's config
    (lr, epochs, batch_size, accum_steps, max_grad_norm, skip_nonfinite_steps, lr_plateau, handle_pool, ema, condition -- the property
    values are each frame's scalar `key=value` entries of its comment line), merged over the suite's finetune_cfg (the
    pipeline wins).  DiffCSPSuite.save_model writes <save_dir>/models/epoch_NNNN every save_freq epochs and <save_dir>/models/final at the
    end: directories that load_model(model_path=...) of this build loads.  `run_rl` is the entry the drop-in's main calls; `reward`,
    `logger` rows and sampling play no part (the logger, when given, receives every epoch's dict).  The MatterGen suite is refused.
    Every models/epoch_NNNN also gets train_state.ckpt (pretrain.save_training_state: raw weights, optimizer, scheduler, counters), written by
    rank 0; resume_from=<such a directory> continues that run, on every rank, as the same run.  With train_cfg.ema set, last.ckpt
    in those directories and in models/final holds the AVERAGED weights -- what the RL pipelines load as their prior -- marked
    "weights": "ema"; the raw weights live in train_state.ckpt."""

    TRAIN_STATE = "train_state.ckpt"

    def __init__(self, model_suite, train_path, save_dir, train_cfg=None, val_path=None, save_freq=10, seed=0, device=None, logger=None,
                 reward=None, resume_from=None, **kwargs):
        from .suite import MatterGenSuite
        if isinstance(model_suite, MatterGenSuite):
            raise ValueError("Pretrain needs the DiffCSP suite: the MatterGen-shaped module has no supervised training here")
        if not train_path:
            raise ValueError("Pretrain: train_path (an extxyz file) is required")
        self.model_suite, self.logger = model_suite, logger
        self.train_path, self.val_path = train_path, val_path
        self.save_dir, self.save_freq, self.seed = save_dir, max(1, int(save_freq)), int(seed)
        self.resume_from = resume_from
        self.device = get_device(device)
        self.cfg = C.create(kwargs)
        self.train_cfg = C.merge(model_suite.finetune_cfg, train_cfg)
        self.models_dir = os.path.join(save_dir, "models")
        os.makedirs(self.models_dir, exist_ok=True)
        self.model, self.history = None, []

    @staticmethod
    def read_dataset(path):
        """An extxyz file -> the CrystalData records pretrain.fit trains on (fractional coordinates wrapped into [0, 1))."""
        from .data import CrystalData
        from .structure import read_extxyz
        out = []
        for s in read_extxyz(path):
            frac = torch.as_tensor(np.asarray(s.frac_coords), dtype=torch.float64) % 1.0
            props = {}
            for k, v in s.info.items():   # the frame's scalar `key=value` entries: what train_cfg.condition.properties may name
                try:
                    props[k] = float(v)
                except ValueError:
                    pass
            out.append(CrystalData(frac.float(), torch.tensor(s.species, dtype=torch.long), torch.tensor([s.lengths], dtype=torch.float32),
                                   torch.tensor([s.angles], dtype=torch.float32), properties=props or None))
        return out

    def load_model(self):
        self.model = self.model_suite.load_model()
        for p in self.model.parameters():
            p.requires_grad = True
        self.model.to(self.device)
        return self.model

    def _save(self, name):
        """models/<name>: the average inside FusedAdam.ema_weights when the run keeps one, the weights themselves otherwise."""
        path = os.path.join(self.models_dir, name)
        opt = self.model.__dict__.get("fit_optimizer")
        if opt is not None and opt.ema_decay is not None:
            with opt.ema_weights(self.model.decoder):
                self.model_suite.save_model(self.model, path, extra={"weights": "ema"})
        else:
            self.model_suite.save_model(self.model, path)
        return path

    def run_rl(self):
        from .pretrain import fit, load_training_state, save_training_state
        rank, _ = rank_world()
        train = self.read_dataset(self.train_path)
        val = self.read_dataset(self.val_path) if self.val_path else None
        if self.model is None:
            self.load_model()
        logging.info(f"training on {len(train)} crystals" + (f", validating on {len(val)}" if val is not None else ""))

        def on_epoch_end(epoch, d):
            if rank != 0:
                return
            if self.logger is not None:
                self.logger.log(dict(d), step=epoch)
            if (epoch + 1) % self.save_freq == 0:
                self._save(f"epoch_{epoch:0>4d}")

        def checkpoint(epoch, state):   # (behind on_epoch_end: the epoch's directory exists)
            save_training_state(os.path.join(self.models_dir, f"epoch_{epoch:0>4d}", self.TRAIN_STATE), state)
        checkpoint.due = lambda epoch: rank == 0 and (epoch + 1) % self.save_freq == 0

        resume = load_training_state(os.path.join(self.resume_from, self.TRAIN_STATE)) if self.resume_from else None
        self.history = fit(self.model, train, self.train_cfg, val_list=val, seed=self.seed, on_epoch_end=on_epoch_end, checkpoint=checkpoint,
                           resume=resume)
        if rank == 0:
            self._save("final")
        return self.history


class TrainPredictor:
    """Train a property predictor (predictor.fit_predictor) on labelled crystals: extxyz in, model directory out -- the
    counterpart of Pretrain for the CSPNet trunk with a scalar head.  train_path / val_path: extxyz files whose frames carry the
    properties as scalar `key=value` entries of the comment line; properties: the names to learn, one head row each; model: the
    PropertyPredictor's arguments (hidden_dim, num_layers, time_dim, num_freqs, ln); train_cfg: fit_predictor's config (lr, epochs,
    batch_size, accum_steps, loss, max_grad_norm, skip_nonfinite_steps, lr_plateau, handle_pool, ema).  predictor.save_predictor writes
    <save_dir>/models/final -- a directory rewards.Surrogate(model_path=...) loads -- holding the averaged weights when train_cfg.ema is
    set.  `run_rl` is the entry the drop-in's main calls; model_suite and reward play no part.  One GPU only."""

    def __init__(self, train_path, save_dir, properties, model=None, train_cfg=None, val_path=None, seed=0, device=None, logger=None,
                 model_suite=None, reward=None, **kwargs):
        if not train_path:
            raise ValueError("TrainPredictor: train_path (an extxyz file) is required")
        names = [properties] if isinstance(properties, str) else [str(p) for p in (properties or [])]
        if not names:
            raise ValueError("TrainPredictor: properties (the names of the frames' key=value entries to learn) is required")
        self.train_path, self.val_path, self.names, self.logger = train_path, val_path, names, logger
        self.save_dir, self.seed = save_dir, int(seed)
        self.device = get_device(device)
        self.model_cfg = C.to_container(C.create(model or {}), resolve=True)
        self.train_cfg = C.create(train_cfg or {})
        self.cfg = C.create(kwargs)
        self.models_dir = os.path.join(save_dir, "models")
        os.makedirs(self.models_dir, exist_ok=True)
        self.model, self.history = None, []

    read_dataset = staticmethod(Pretrain.read_dataset)

    def load_model(self):
        from .predictor import PropertyPredictor
        self.model = PropertyPredictor(self.names, device=self.device, seed=self.seed, **self.model_cfg)
        return self.model

    def _save(self, name):
        from .predictor import save_predictor
        path = os.path.join(self.models_dir, name)
        opt = self.model.__dict__.get("fit_optimizer")
        if opt is not None and opt.ema_decay is not None:
            with opt.ema_weights(self.model):
                return save_predictor(self.model, path)
        return save_predictor(self.model, path)

    def run_rl(self):
        from .predictor import fit_predictor
        train = self.read_dataset(self.train_path)
        val = self.read_dataset(self.val_path) if self.val_path else None
        if self.model is None:
            self.load_model()
        logging.info(f"training a predictor of {self.names} on {len(train)} crystals" + (f", validating on {len(val)}" if val is not None else ""))

        def on_epoch_end(epoch, d):
            if self.logger is not None:
                self.logger.log(dict(d), step=epoch)
        self.history = fit_predictor(self.model, train, self.train_cfg, val_list=val, seed=self.seed, on_epoch_end=on_epoch_end)
        self._save("final")
        return self.history
