#!/usr/bin/env python
"""Continual-learning driver for VAR-GP on MI355X — counterpart of the reference's
`experiments/vargp.py` (train :14-73, toy :76-104, split_mnist :107-140, permuted_mnist :143-186).

Same commands, flags and defaults:

    python experiments/vargp.py toy      [--epochs 5000 --M 20 --lr 1e-2 --beta 1.0 ...]
    python experiments/vargp.py s-mnist  [--epochs 500  --M 60 --lr 3e-3 --beta 10.0 ...]
    python experiments/vargp.py p-mnist  [--n_tasks 10 --epochs 1000 --M 100 --lr 3.7e-3 --beta 1.64 ...]

Differences: wandb / tensorboard / fire are optional (a JSONL logger under --log_dir is always written);
MNIST is read from IDX files under --data_dir if present, else an MNIST-shaped synthetic surrogate is used
(no network); --graph replays the training step from a captured hipGraph; the training data live in HBM and are shuffled and
gathered on the device (--dataloader restores the reference's host-side DataLoader); `toy --retrain` is the counterpart of the
reference's experiments/vargp_retrain.py (VARGPRetrain).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from torch.utils.data import ConcatDataset, DataLoader  # noqa: E402

import vargp_amd  # noqa: E402
from vargp_amd.datasets import PermutedMNIST, SplitMNIST, ToyDataset  # noqa: E402
from vargp_amd.train import ElboTrainer  # noqa: E402
from vargp_amd.train_utils import (DeviceBatches, EarlyStopper, compute_accuracy, compute_loo, compute_lpd,  # noqa: E402
                                   compute_uncertainty, set_seeds)
from vargp_amd.vargp import VARGP, _CLF_Q_INITS  # noqa: E402


class JsonlLogger:
    """add_scalar()-compatible logger (the reference uses a tensorboard SummaryWriter)."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.log_dir = log_dir
        self._f = open(os.path.join(log_dir, 'scalars.jsonl'), 'a')

    def add_scalar(self, key, value, global_step=None):
        self._f.write(json.dumps(dict(key=key, value=float(value), step=global_step, t=time.time())) + '\n')
        self._f.flush()

    def close(self):
        self._f.close()


def train(task_id, train_set, val_set, test_set, ep_var_mean=True, map_est_hypers=False, dkl=False,
          epochs=1, M=20, n_f=10, n_var_samples=3, batch_size=512, lr=1e-2, beta=1.0,
          eval_interval=10, patience=20, prev_params=None, logger=None, device=None, graph=False, seed=None,
          retrain=False, eval_shared_hypers=False, dataloader=False, kernel='rbf', native_kernel=False,
          likelihood='softmax', link='probit', lpd=False, z_init='random', kmeans_iters=20, lengthscale_init='default',
          uncertainty=False, greedy_candidates=4096, q_init='default', newton_iters=20, em_rounds=5, em_steps=20,
          site_samples=32, loo=False):
    if retrain:      # the variant of experiments/vargp_retrain.py:14-19 (earlier tasks' inducing parameters re-optimised)
        from vargp_amd.vargp_retrain import VARGPRetrain
        assert kernel == 'rbf', '--retrain builds its model with the RBF kernel'
        assert z_init == 'random' and lengthscale_init == 'default', "--retrain builds its model with the reference's initialisation"
        assert q_init == 'default', "--retrain builds its model with the reference's initialisation"
        gp = VARGPRetrain.create_clf(train_set, M=M, n_f=n_f, n_var_samples=n_var_samples, prev_params=prev_params,
                                     likelihood=likelihood, link=link).to(device)
        graph = False
    else:
        gp = VARGP.create_clf(train_set, M=M, n_f=n_f, n_var_samples=n_var_samples, prev_params=prev_params,
                              ep_var_mean=ep_var_mean, map_est_hypers=map_est_hypers, dkl=dkl, kernel=kernel,
                              native_kernel=native_kernel, likelihood=likelihood, link=link, z_init=z_init,
                              kmeans_iters=kmeans_iters, lengthscale_init=lengthscale_init,
                              greedy_candidates=greedy_candidates, q_init=q_init, newton_iters=newton_iters, em_rounds=em_rounds,
                              em_steps=em_steps, site_samples=site_samples).to(device)
    stopper = EarlyStopper(patience=patience)
    N = len(train_set)
    # the program's counter-based noise generator is keyed by the run's seed (the reference draws from the torch global
    # generator that set_seeds controls, train_utils.py:13-19): replicates with different seeds see different noise
    noise_seed = (int(seed) if seed is not None else torch.initial_seed()) * 1000003 + task_id
    trainer = ElboTrainer(gp, lr=lr, beta=beta, n_total=N, noise_seed=noise_seed & 0x7FFFFFFFFFFFFFFF)   # Yogi (:23)
    # Default: the data set lives in HBM, one on-device permutation per epoch, minibatches gathered on the device (no host
    # copy, no host sync inside an epoch).  --dataloader: the reference's `DataLoader(train_set, batch_size, shuffle=True)`
    # (experiments/vargp.py:26) over host tensors -- same batches-per-epoch semantics (ragged last batch included), ~8 ms of
    # host work per 512-sample batch against a 0.24 ms device step.
    loader = DataLoader(train_set, batch_size=batch_size, shuffle=True) if dataloader else \
        DeviceBatches(train_set, batch_size, device, shuffle=True)
    captured = set()         # minibatch sizes with a captured step: the full batch and the ragged last one of an epoch
    n_steps, t_train = 0, 0.0

    # --graph on the device-resident loader: the epoch's full minibatches run as graphs of K steps whose steps gather their own
    # minibatch (ElboTrainer.capture_epoch / run_epoch: the batch index advances on the device); the ragged last batch and every
    # other combination (--dataloader, no --graph, trainers without a device-side step count) take the per-step loop below
    epoch_graphs = graph and not dataloader and N >= batch_size and os.environ.get('VARGP_EPOCH_GRAPHS', '1') != '0'

    for e in range(epochs):
        torch.cuda.synchronize()
        t_epoch = time.perf_counter()
        batches = loader
        if epoch_graphs:
            order = loader.epoch_order()
            if batch_size not in captured:
                torch.cuda.synchronize()
                t_cap = time.perf_counter()
                trainer.capture(*loader.take(order[:batch_size]))
                if trainer.capture_epoch(loader.data, loader.targets) is None:
                    epoch_graphs = False
                torch.cuda.synchronize()
                t_epoch += time.perf_counter() - t_cap              # the one-off captures are not part of the training rate
                captured.add(batch_size)
            if epoch_graphs:
                (kl_hypers, kl_u, lik), done = trainer.run_epoch(order)
                n_steps += done
                batches = [order[done * batch_size:]] if done * batch_size < N else []
            else:
                batches = [order[i:i + batch_size] for i in range(0, N, batch_size)]
        for item in batches:
            if dataloader:
                x, y = item[0].to(device), item[1].to(device)
                nb = x.size(0)
            else:
                nb = item.numel()
            if graph:
                if nb not in captured:
                    torch.cuda.synchronize()
                    t_cap = time.perf_counter()
                    trainer.capture(*(loader.take(item) if not dataloader else (x, y)))
                    torch.cuda.synchronize()
                    t_train -= time.perf_counter() - t_cap        # the one-off capture is not part of the training rate
                    captured.add(nb)
                if dataloader:
                    kl_hypers, kl_u, lik = trainer.step_graph(x, y)
                else:
                    kl_hypers, kl_u, lik = trainer.step_graph_gather(loader.data, loader.targets, item)
            else:
                kl_hypers, kl_u, lik = trainer.step(*(loader.take(item) if not dataloader else (x, y)))
            n_steps += 1
        # ('defer' mode: the count of failed factorisations rides in front of the epoch's sync, read after it)
        failed = vargp_amd.linalg_error_count_begin() if graph else None
        torch.cuda.synchronize()             # the one host sync of the epoch
        t_train += time.perf_counter() - t_epoch
        if e == 0 and epochs > 1:            # the first epoch pays the one-off costs (kernel module loads, first allocations,
            n_steps, t_train = 0, 0.0        # program workspaces): the logged rate is the steady state of the later epochs
        if graph and int(failed):
            # 'defer' mode never syncs inside a step: failed factorisations are NaN-filled and flagged on the device.
            # The reference raises at once (torch.cholesky, gp_utils.py:10); here the check runs once per epoch.
            raise torch.linalg.LinAlgError(f'task {task_id}, epoch {e + 1}: a Cholesky factorisation met a matrix that is '
                                           'not positive-definite')

        if (e + 1) % eval_interval == 0:
            acc_summary = {
                f'task{task_id}/train/acc': compute_accuracy(train_set, gp, device=device, shared_hypers=eval_shared_hypers),
                f'task{task_id}/val/acc': compute_accuracy(val_set, gp, device=device, shared_hypers=eval_shared_hypers),
                f'task{task_id}/test/acc': compute_accuracy(test_set, gp, device=device, shared_hypers=eval_shared_hypers),
            }
            loss_summary = {
                f'task{task_id}/loss/kl_hypers': kl_hypers.item(),
                f'task{task_id}/loss/kl_u': kl_u.item(),
                f'task{task_id}/loss/lik': lik.item(),
            }
            if lpd:      # --lpd: mean held-out log predictive density of the test set (every task seen so far)
                loss_summary[f'task{task_id}/test/lpd'] = compute_lpd(test_set, gp, device=device,
                                                                      shared_hypers=eval_shared_hypers)
            if uncertainty:      # --uncertainty: mean predictive entropy of the same test set and its epistemic part (nats)
                ent, _, mi = compute_uncertainty(test_set, gp, device=device, shared_hypers=eval_shared_hypers)
                loss_summary[f'task{task_id}/test/entropy'], loss_summary[f'task{task_id}/test/mi'] = ent, mi
            if logger is not None:
                for k, v in dict(**loss_summary, **acc_summary).items():
                    logger.add_scalar(k, v, global_step=e + 1)
            stopper(acc_summary[f'task{task_id}/val/acc'],
                    dict(state_dict=gp.state_dict(), acc_summary=acc_summary, step=e + 1))
            if stopper.is_done():
                break

    if loo:      # --loo: mean leave-one-out log predictive density of THIS task's training set under the trained q(u) (VARGP.loo)
        kw = dict(n_f=site_samples) if likelihood == 'softmax' else {}
        loo_lpd, n_unstable = compute_loo(train_set, gp, device=device, **kw)
        print(f'task {task_id}: mean LOO lpd {loo_lpd:.4f} over {N - n_unstable} of {N} training points ({n_unstable} unstable)')
        if logger is not None:
            logger.add_scalar(f'task{task_id}/train/loo_lpd', loo_lpd, global_step=n_steps)
            logger.add_scalar(f'task{task_id}/train/loo_unstable', n_unstable, global_step=n_steps)

    info = stopper.info() or dict(state_dict=gp.state_dict(), acc_summary={}, step=epochs)
    if logger is not None and n_steps:
        # end-to-end training rate of this task: steps / wall time of the epochs' training loops (evaluation excluded)
        logger.add_scalar(f'task{task_id}/train/steps_per_s', n_steps / max(t_train, 1e-9), global_step=n_steps)
    if logger is not None:
        for k, v in info.get('acc_summary').items():
            logger.add_scalar(f'{k}_best', v, global_step=info.get('step'))
        torch.save(info.get('state_dict'), os.path.join(logger.log_dir, f'ckpt{task_id}.pt'))
    return info.get('state_dict')


def _setup(args):
    set_seeds(args.seed)
    vargp_amd.set_cholesky_error_mode('defer' if args.graph else 'raise')
    device = 'cuda' if torch.cuda.is_available() else None
    if device is None:
        raise SystemExit('vargp_amd needs a ROCm GPU (there is no CPU path)')
    return device, JsonlLogger(args.log_dir)


def toy(args):
    device, logger = _setup(args)
    toy_train = ToyDataset()
    toy_val = ToyDataset(X=toy_train.data.clone(), Y=toy_train.targets.clone())
    toy_test = ToyDataset(X=toy_train.data.clone(), Y=toy_train.targets.clone())
    prev_params = []
    for t in range(2):
        toy_train.filter_by_class([2 * t, 2 * t + 1])
        toy_val.filter_by_class(range(2 * t + 2))
        toy_test.filter_by_class(range(2 * t + 2))
        sd = train(t, toy_train, toy_val, toy_test, epochs=args.epochs, M=args.M, lr=args.lr, beta=args.beta,
                   batch_size=args.batch_size, ep_var_mean=args.ep_var_mean, map_est_hypers=args.map_est_hypers,
                   dkl=args.dkl, kernel=args.kernel, native_kernel=args.native_kernel, likelihood=args.likelihood,
                   link=args.link, prev_params=prev_params, logger=logger, device=device, patience=-1,
                   eval_interval=args.eval_interval, graph=args.graph, seed=args.seed, retrain=args.retrain,
                   eval_shared_hypers=args.eval_shared_hypers, n_var_samples=args.n_var_samples, dataloader=args.dataloader,
                   lpd=args.lpd, z_init=args.z_init, kmeans_iters=args.kmeans_iters, lengthscale_init=args.lengthscale_init, q_init=args.q_init,
                   newton_iters=args.newton_iters, em_rounds=args.em_rounds, em_steps=args.em_steps, site_samples=args.site_samples,
                   uncertainty=args.uncertainty, greedy_candidates=args.greedy_candidates, loo=args.loo)
        prev_params.append(sd)
    logger.close()


def split_mnist(args):
    device, logger = _setup(args)
    syn = dict(synthetic=args.synthetic, n_synth=args.n_synth)
    mnist_train = SplitMNIST(args.data_dir, train=True, **syn)
    mnist_val = SplitMNIST(args.data_dir, train=True, **syn)
    mnist_test = SplitMNIST(args.data_dir, train=False, synthetic=args.synthetic,
                            n_synth=args.n_synth // 6 if args.n_synth else None)
    idx = torch.randperm(len(mnist_train))
    n_val = max(len(idx) // 6, 1)
    mnist_train.filter_by_idx(idx[:-n_val])
    mnist_val.filter_by_idx(idx[-n_val:])
    prev_params = []
    for t in range(5):
        mnist_train.filter_by_class([2 * t, 2 * t + 1])
        mnist_val.filter_by_class(range(2 * t + 2))
        mnist_test.filter_by_class(range(2 * t + 2))
        sd = train(t, mnist_train, mnist_val, mnist_test, epochs=args.epochs, M=args.M, lr=args.lr, beta=args.beta,
                   batch_size=args.batch_size, ep_var_mean=args.ep_var_mean, map_est_hypers=args.map_est_hypers,
                   dkl=args.dkl, kernel=args.kernel, native_kernel=args.native_kernel, likelihood=args.likelihood,
                   link=args.link, prev_params=prev_params, logger=logger, device=device,
                   eval_interval=args.eval_interval, graph=args.graph, seed=args.seed,
                   eval_shared_hypers=args.eval_shared_hypers, n_var_samples=args.n_var_samples, dataloader=args.dataloader,
                   lpd=args.lpd, z_init=args.z_init, kmeans_iters=args.kmeans_iters, lengthscale_init=args.lengthscale_init, q_init=args.q_init,
                   newton_iters=args.newton_iters, em_rounds=args.em_rounds, em_steps=args.em_steps, site_samples=args.site_samples,
                   uncertainty=args.uncertainty, greedy_candidates=args.greedy_candidates, loo=args.loo)
        prev_params.append(sd)
    logger.close()


def permuted_mnist(args):
    device, logger = _setup(args)
    syn = dict(synthetic=args.synthetic, n_synth=args.n_synth)
    tasks = [torch.arange(784)] + PermutedMNIST.create_tasks(n=args.n_tasks - 1)   # first task is unpermuted
    base = PermutedMNIST(args.data_dir, train=True, **syn)
    idx = torch.randperm(len(base))
    n_val = max(len(idx) // 6, 1)
    train_idx, val_idx = idx[:-n_val], idx[-n_val:]
    mnist_val, mnist_test, prev_params = [], [], []
    for t in range(len(tasks)):
        mnist_train = PermutedMNIST(args.data_dir, train=True, **syn)
        mnist_train.filter_by_idx(train_idx)
        mnist_train.set_task(tasks[t])
        mnist_val.append(PermutedMNIST(args.data_dir, train=True, **syn))
        mnist_val[-1].filter_by_idx(val_idx)
        mnist_val[-1].set_task(tasks[t])
        mnist_test.append(PermutedMNIST(args.data_dir, train=False, synthetic=args.synthetic,
                                        n_synth=args.n_synth // 6 if args.n_synth else None))
        mnist_test[-1].set_task(tasks[t])
        sd = train(t, mnist_train, ConcatDataset(mnist_val), ConcatDataset(mnist_test), epochs=args.epochs, M=args.M,
                   lr=args.lr, beta=args.beta, batch_size=args.batch_size, ep_var_mean=args.ep_var_mean,
                   map_est_hypers=args.map_est_hypers, dkl=args.dkl, kernel=args.kernel, native_kernel=args.native_kernel, likelihood=args.likelihood,
                   link=args.link, prev_params=prev_params, logger=logger,
                   device=device, eval_interval=args.eval_interval, graph=args.graph, seed=args.seed,
                   eval_shared_hypers=args.eval_shared_hypers, n_var_samples=args.n_var_samples, dataloader=args.dataloader,
                   lpd=args.lpd, z_init=args.z_init, kmeans_iters=args.kmeans_iters, lengthscale_init=args.lengthscale_init, q_init=args.q_init,
                   newton_iters=args.newton_iters, em_rounds=args.em_rounds, em_steps=args.em_steps, site_samples=args.site_samples,
                   uncertainty=args.uncertainty, greedy_candidates=args.greedy_candidates, loo=args.loo)
        prev_params.append(sd)
    logger.close()


def parse_args(argv=None):
    defaults = {   # reference defaults: experiments/vargp.py:76-78,107-109,143-145
        'toy': dict(epochs=5000, M=20, lr=1e-2, beta=1.0),
        's-mnist': dict(epochs=500, M=60, lr=3e-3, beta=10.0),
        'p-mnist': dict(epochs=1000, M=100, lr=3.7e-3, beta=1.64),
    }
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name, d in defaults.items():
        sp = sub.add_parser(name, aliases=[name.replace('-', '_')])
        sp.add_argument('--data_dir', default=os.environ.get('USER_DATADIR', '/tmp'))
        sp.add_argument('--epochs', type=int, default=d['epochs'])
        sp.add_argument('--M', type=int, default=d['M'])
        sp.add_argument('--lr', type=float, default=d['lr'])
        sp.add_argument('--batch_size', type=int, default=512)
        sp.add_argument('--beta', type=float, default=d['beta'])
        sp.add_argument('--ep_var_mean', type=lambda v: str(v).lower() not in ('0', 'false'), default=True)
        sp.add_argument('--map_est_hypers', type=lambda v: str(v).lower() not in ('0', 'false'), default=False)
        sp.add_argument('--dkl', type=lambda v: str(v).lower() not in ('0', 'false'), default=False)
        sp.add_argument('--kernel', choices=('rbf', 'matern12', 'matern32', 'matern52'), default='rbf',
                        help='covariance function (not stored in checkpoints: give it again when reloading one)')
        sp.add_argument('--native_kernel', action='store_true',
                        help='run a Matern model on the native block ELBO program instead of the composed per-op route '
                             '(needs --kernel matern12 / matern32 / matern52 and no --dkl; not stored in checkpoints)')
        sp.add_argument('--likelihood', choices=('softmax', 'bernoulli'), default='softmax',
                        help="classification likelihood: the reference's Monte-Carlo softmax, or independent one-vs-rest "
                             'Bernoulli outputs (deterministic 20-node Gauss-Hermite rule; not stored in checkpoints)')
        sp.add_argument('--link', choices=('probit', 'logit'), default='probit',
                        help='link function of --likelihood bernoulli')
        sp.add_argument('--z_init', choices=('random', 'kmeans', 'greedy'), default='random',
                        help="inducing points of a new task: M random data points per output (the reference's), the "
                             'k-means centres of the task found from them on the device, or greedy conditional-variance '
                             "selection under the model's kernel, started from the earlier tasks' inducing points (not with --dkl)")
        sp.add_argument('--greedy_candidates', type=int, default=4096,
                        help='random data points per output that --z_init greedy selects among (at most)')
        sp.add_argument('--kmeans_iters', type=int, default=20, help='Lloyd iterations of --z_init kmeans (at most)')
        sp.add_argument('--lengthscale_init', choices=('default', 'median'), default='default',
                        help="lengthscales of the first task: 0.5 (the reference's), or the median distance between pairs of "
                             'its points (not with --dkl)')
        sp.add_argument('--q_init', choices=_CLF_Q_INITS, default='default',
                        help="q(u) of each task: the reference's start, fit_q_newton_ on the task's whole training set, or "
                             'fit_sites_ (variational EM: inducing points and kernel hyper-parameters move too) '
                             '(--likelihood bernoulli only), or fit_q_softmax_ / fit_softmax_sites_ (its variational EM) '
                             '(--likelihood softmax only)')
        sp.add_argument('--newton_iters', type=int, default=20, help='iterations of --q_init newton / of an E-step of em (at most)')
        sp.add_argument('--site_samples', type=int, default=32, help='draws per point of --q_init newton_softmax / em_softmax')
        sp.add_argument('--em_rounds', type=int, default=5, help='rounds of --q_init em / em_softmax')
        sp.add_argument('--em_steps', type=int, default=20, help='Yogi steps per M-step of --q_init em / em_softmax')
        sp.add_argument('--seed', type=int, default=None)
        sp.add_argument('--eval_interval', type=int, default=10)
        sp.add_argument('--log_dir', default=os.path.join('runs', f'{name}-{int(time.time())}'))
        sp.add_argument('--synthetic', action='store_true', default=None,
                        help='force the MNIST-shaped synthetic surrogate (default: only if IDX files are missing)')
        sp.add_argument('--n_synth', type=int, default=None, help='size of the synthetic training set')
        sp.add_argument('--graph', action='store_true', help='replay the training step from a captured hipGraph')
        sp.add_argument('--dataloader', action='store_true',
                        help="feed the steps from the reference's torch DataLoader over host tensors instead of the "
                             'device-resident epochs (on-device permutation + gather)')
        sp.add_argument('--n_var_samples', type=int, default=3,
                        help='Monte-Carlo samples of the kernel hyper-parameters per step (reference: fixed at 3, '
                             'experiments/vargp.py:16; BASELINE config 3 quotes 10)')
        sp.add_argument('--eval_shared_hypers', action='store_true',
                        help='accuracy sweeps draw the kernel hyper-parameters once per data set (one factorisation of '
                             'K(z_<=t) per sweep) instead of once per batch as the reference does')
        sp.add_argument('--lpd', action='store_true',
                        help='also log test/lpd at every evaluation: the mean held-out log predictive density per point of '
                             'the test set of the tasks seen so far (VARGP.log_prob)')
        sp.add_argument('--uncertainty', action='store_true',
                        help='also log test/entropy and test/mi at every evaluation: the mean predictive entropy per point of '
                             'the test set of the tasks seen so far and its epistemic part, the mutual information of the '
                             'label and the model (VARGP.uncertainty; nats)')
        sp.add_argument('--loo', action='store_true',
                        help="after each task's training, print (and log as train/loo_lpd) the mean leave-one-out log predictive "
                             "density of the task's training set under the trained q(u) (VARGP.loo: the cavity of the Gaussian "
                             'sites at theta = log_mean, no refits; exact only at a fixed point of the site iteration, so the '
                             'points whose cavity is improper after minibatch training are counted as unstable and left out '
                             'of the mean); needs --ep_var_mean true and no --retrain')
        if name == 'toy':
            sp.add_argument('--retrain', action='store_true',
                            help='VARGPRetrain (reference: experiments/vargp_retrain.py toy): re-optimise the earlier '
                                 "tasks' inducing parameters")
        if name == 'p-mnist':
            sp.add_argument('--n_tasks', type=int, default=10)
    args = ap.parse_args(argv)
    if args.native_kernel and (args.kernel == 'rbf' or args.dkl or getattr(args, 'retrain', False)):
        ap.error('--native_kernel selects the native route of a Matern kernel: it needs --kernel matern12 / matern32 / matern52 '
                 'and neither --dkl nor --retrain')
    if args.loo and (not args.ep_var_mean or getattr(args, 'retrain', False)):
        ap.error('--loo reads q(u_t) as prior x Gaussian sites: it needs --ep_var_mean true and no --retrain')
    if args.graph and args.likelihood == 'bernoulli':
        ap.error('--graph with --likelihood bernoulli: the epoch graphs (capture_epoch / step_graph_gather) run the softmax '
                 'likelihood inside the native program and refuse a Bernoulli model; train it without --graph')
    return args


def main(argv=None):
    args = parse_args(argv)
    {'toy': toy, 's-mnist': split_mnist, 's_mnist': split_mnist, 'p-mnist': permuted_mnist,
     'p_mnist': permuted_mnist}[args.cmd](args)


if __name__ == '__main__':
    main()
