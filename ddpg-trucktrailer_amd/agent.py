"""DDPG agent with the reference's interface (DDPG/DDPG_agent.py:9-131) on PyTorch-ROCm.

    Agent(alpha, beta, input_dims, tau, n_actions, gamma, max_size, fc1_dims, fc2_dims, batch_size)
    .choose_action(observation, evaluate) .remember(s, a, r, s_, done) .learn()
    .save_models() .load_models() .save_models_progress(success) .update_network_parameters(tau)

learn() keeps the reference's order of operations (DDPG_agent.py:72-106): targets from the target nets,
critic MSE step, THEN the actor step through the already-updated critic, then the soft update of every
named parameter (LayerNorm included).  `learn_batch` is the same update on an explicit device batch; it is
what the N-env loop (rollout.py) captures into a hipGraph and where the data-parallel gradient all-reduce
sits (two sites: before critic.optimizer.step and before actor.optimizer.step)."""
import numpy as np
import torch as T
import torch.nn.functional as F

from ddpg_trucktrailer_amd.networks import ActorNetwork, CriticNetwork
from ddpg_trucktrailer_amd.noise import OUActionNoise
from ddpg_trucktrailer_amd.replay_buffer import ReplayBuffer


class GradAllReduce:
    """Flat-bucket gradient averaging over the data-parallel group (RCCL over xGMI on GPUs, gloo on CPU).
    One all-reduce per network per learn(): critic 132,201 f32 = 529 KB, actor 131,601 f32 = 526 KB."""

    def __init__(self, params, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.params = [p for p in params]
        self.world = dist.get_world_size(group)
        n = sum(p.numel() for p in self.params)
        self.flat = T.zeros(n, dtype=self.params[0].dtype, device=self.params[0].device)
        self.views, off = [], 0
        for p in self.params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()

    def __call__(self):
        T._foreach_copy_(self.views, [p.grad for p in self.params])
        self.dist.all_reduce(self.flat, op=self.dist.ReduceOp.SUM, group=self.group)
        self.flat.div_(self.world)
        T._foreach_copy_([p.grad for p in self.params], self.views)


class Agent():
    def __init__(self, alpha, beta, input_dims, tau, n_actions, gamma=0.99,
                 max_size=1000000, fc1_dims=400, fc2_dims=300,
                 batch_size=64, device=None, chkpt_dir='tmp/ddpg', capturable=False, replay=True, td3=None, loss_shape=None,
                 demo_loss=None, grad_clip=None):
        """td3: None = DDPG, line for line; a td3.TD3Config = TD3 (Fujimoto et al., 2018): a second critic `critic_2` with its target
        `target_critic_2`, target-policy smoothing, and the actor and all targets updated on every policy_delay-th update only.
        loss_shape: None = the MSE critic loss and the plain actor loss; a loss_shape.LossShape = the Huber critic loss and / or the
        actor's pre-activation penalty c mean(pre^2) in learn_batch.  Not with td3.
        demo_loss: None, or a demo_loss.DemoLoss = a behaviour-cloning term on the rows learn_batch is told are demonstrations
        (demo_rows=), gated by a Q-filter.  Composes with loss_shape.  Not with td3.
        grad_clip: None, or a grad_clip.GradClip = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm) between the gradient and
        optimizer.step() at each site that has a value.  Not with td3."""
        if grad_clip is not None:
            from ddpg_trucktrailer_amd.grad_clip import check_grad_clip
            check_grad_clip(grad_clip, td3=td3)
        self.grad_clip = grad_clip
        if demo_loss is not None:
            from ddpg_trucktrailer_amd.demo_loss import check_demo_loss
            check_demo_loss(demo_loss, td3=td3)
        self.demo_loss = demo_loss
        self.last_demo_mask = None       # [B] bool: the rows the last learn_batch applied the cloning term to
        if loss_shape is not None:
            from ddpg_trucktrailer_amd.loss_shape import check_loss_shape
            check_loss_shape(loss_shape, td3=td3)
        self.loss_shape = loss_shape
        self.gamma, self.tau, self.batch_size, self.alpha, self.beta = gamma, tau, batch_size, alpha, beta
        self.device = T.device(device) if device is not None else T.device('cuda:0' if T.cuda.is_available() else 'cpu')
        self.memory = ReplayBuffer(max_size, input_dims, n_actions, device=self.device) if replay else None
        self.noise = OUActionNoise(mu=np.zeros(n_actions))
        kw = dict(device=self.device, chkpt_dir=chkpt_dir, capturable=capturable)
        self.actor = ActorNetwork(alpha, input_dims, fc1_dims, fc2_dims, n_actions=n_actions, name='actor', **kw)
        self.critic = CriticNetwork(beta, input_dims, fc1_dims, fc2_dims, n_actions=n_actions, name='critic', **kw)
        self.target_actor = ActorNetwork(alpha, input_dims, fc1_dims, fc2_dims, n_actions=n_actions,
                                         name='target_actor', **kw)
        self.target_critic = CriticNetwork(beta, input_dims, fc1_dims, fc2_dims, n_actions=n_actions,
                                           name='target_critic', **kw)
        self.td3 = td3
        if td3 is not None:
            self.critic_2 = CriticNetwork(beta, input_dims, fc1_dims, fc2_dims, n_actions=n_actions, name='critic_2', **kw)
            self.target_critic_2 = CriticNetwork(beta, input_dims, fc1_dims, fc2_dims, n_actions=n_actions,
                                                 name='target_critic_2', **kw)
            self._critic_2_params = list(self.critic_2.parameters())
            self.td3_updates = 0                 # critic updates done (a full update is every policy_delay-th)
            self._td3_gen = T.Generator(device=self.device)
            self.seed_td3_noise(0)
        self.update_network_parameters(tau=1)
        self._critic_params = list(self.critic.parameters())
        self._actor_params = list(self.actor.parameters())
        self.grad_sync_actor = self.grad_sync_critic = None
        self.fused_targets = False
        self.fused_learner = None      # set by DDPGRollout when learn() runs on the hand-fused kernels
        self.last_critic_loss = self.last_actor_loss = None

    # ------------------------------------------------------------------ acting (DDPG_agent.py:36-49)
    def choose_action(self, observation, evaluate=False):
        self.actor.eval()
        state = T.as_tensor(np.asarray([observation]), dtype=T.float).to(self.device)
        with T.no_grad():
            mu = self.actor.forward(state)
        if not evaluate:
            mu = mu + T.tensor(self.noise(), dtype=T.float).to(self.device)
        self.actor.train()
        return mu.cpu().detach().numpy()[0]

    def remember(self, state, action, reward, state_, done):
        self.memory.store_transition(state, action, reward, state_, done)

    # ------------------------------------------------------------------ checkpoints (DDPG_agent.py:54-70)
    def _nets(self):
        nets = (self.actor, self.target_actor, self.critic, self.target_critic)
        return nets + (self.critic_2, self.target_critic_2) if self.td3 is not None else nets

    def save_models(self):
        for net in self._nets():
            net.save_checkpoint()

    def save_models_progress(self, success):
        for net in self._nets():
            net.save_checkpoint_progress(success=success)

    def load_models(self):
        for net in self._nets():
            net.load_checkpoint()

    # ------------------------------------------------------------------ learning (DDPG_agent.py:72-106)
    def enable_data_parallel(self, group=None):
        """Average gradients over the process group at the two optimizer sites; broadcast rank 0's weights."""
        import torch.distributed as dist
        for net in self._nets():
            for p in net.parameters():
                dist.broadcast(p.data, src=0, group=group)
        self.grad_sync_critic = GradAllReduce(self.critic.parameters(), group)
        self.grad_sync_actor = GradAllReduce(self.actor.parameters(), group)

    def learn(self):
        if self.memory.mem_cntr < self.batch_size:
            return
        states, actions, rewards, states_, done = self.memory.sample_buffer(self.batch_size)
        self.learn_batch(states, actions, rewards, states_, done)

    def learn_batch(self, states, actions, rewards, states_, done, discount=None, eps=None, full=None, demo_rows=None,
                    label_rows=None, labels=None):
        # discount: what multiplies q' in the target (default gamma); gamma ** n for a batch of n-step tuples (TrajectoryRing.sample)
        # eps, full: TD3 only (see _learn_batch_td3)
        # demo_rows (with demo_loss): [B] bool, the rows that are demonstrations (None: none is)
        # label_rows, labels (with demo_loss; together): [B] bool and [B] f32 -- on a labelled row the cloning target is the label
        # (the expert's decision on the row's state) and the Q-filter is skipped; it wins over demo_rows
        discount = self.gamma if discount is None else discount
        demo = self.demo_loss
        if demo_rows is not None and demo is None:
            raise ValueError("demo_rows without demo_loss (Agent(demo_loss=...))")
        if (label_rows is None) != (labels is None):
            raise ValueError("label_rows and labels go together ([B] bool and [B] f32)")
        if label_rows is not None and demo is None:
            raise ValueError("label_rows without demo_loss (Agent(demo_loss=...))")
        if label_rows is not None and self.td3 is not None:
            raise ValueError("label_rows with td3 is not supported")
        if self.td3 is not None:
            return self._learn_batch_td3(states, actions, rewards, states_, done, discount, eps, full)
        with T.no_grad():
            if self.fused_targets:      # one fused f32-MFMA launch per target net (csrc/ttnet.hip)
                from ddpg_trucktrailer_amd import fused
                target_actions = fused.actor_forward(self.target_actor, states_)
                critic_value_ = fused.critic_forward(self.target_critic, states_, target_actions)
            else:
                target_actions = self.target_actor.forward(states_)
                critic_value_ = self.target_critic.forward(states_, target_actions)
            critic_value_ = critic_value_.masked_fill(done.view(-1, 1), 0.0).view(-1)      # critic_value_[done] = 0.0
            target = (rewards + discount * critic_value_).view(-1, 1)
        critic_value = self.critic.forward(states, actions)

        # Gradients through torch.autograd.grad, not .backward(): backward() delivers them through each parameter's
        # AccumulateGrad node, which is pinned to the stream it was first used on -- a node kept alive from another stream
        # (e.g. by a clone of the parameter that still carries its grad_fn) forks a hipGraph capture of this function and
        # HIP's EndCapture then crashes the process.  grad() returns the same numbers without touching those nodes.
        shape = self.loss_shape
        if shape is not None and shape.huber_delta is not None:
            critic_loss = F.huber_loss(critic_value, target, delta=shape.huber_delta)      # (half the MSE gradient inside the zone)
        else:
            critic_loss = F.mse_loss(target, critic_value)
        for p, g in zip(self._critic_params, T.autograd.grad(critic_loss, self._critic_params)):
            p.grad = g                                       # zero_grad(set_to_none=True) + backward()
        if self.grad_sync_critic is not None:
            self.grad_sync_critic()
        clip = self.grad_clip
        if clip is not None and clip.critic is not None:
            T.nn.utils.clip_grad_norm_(self._critic_params, clip.critic)
        self.critic.optimizer.step()

        # The actor step differentiates -Q(s, mu(s)) through the ALREADY UPDATED critic.  The reference lets
        # that backward also deposit gradients in the critic's parameters and throws them away at the next
        # zero_grad (DDPG_agent.py:95,100-104); asking for the actor's gradients only changes nothing the optimizers see.
        if shape is not None and shape.pre_penalty > 0:
            mu, pre = self.actor.forward_pre(states)
            q_pi = self.critic.forward(states, mu)
            actor_loss = T.mean(-q_pi) + shape.pre_penalty * T.mean(pre * pre)
        else:
            mu = self.actor.forward(states)
            q_pi = self.critic.forward(states, mu)
            actor_loss = T.mean(-q_pi)
        if demo is not None and (demo_rows is not None or label_rows is not None):
            # the cloning term on the demonstration rows [that pass the Q-filter]: q = Q(s, a) of the forward that PRECEDED the
            # critic step, q_pi = Q(s, mu(s)) through the UPDATED critic -- one Adam step apart (demo_loss.py); strict, NaN = out
            with T.no_grad():
                m = (demo_rows.view(-1).to(device=mu.device, dtype=T.bool) if demo_rows is not None
                     else T.zeros(mu.shape[0], dtype=T.bool, device=mu.device))
                if demo.q_filter:
                    m = m & (critic_value.view(-1) > q_pi.view(-1))
                target_a = actions.view(-1)
                if label_rows is not None:
                    lab = label_rows.view(-1).to(device=mu.device, dtype=T.bool)
                    m = m | lab
                    target_a = T.where(lab, labels.view(-1).to(device=mu.device, dtype=mu.dtype), target_a)
            self.last_demo_mask = m
            d = mu.view(-1) - target_a
            actor_loss = actor_loss + demo.bc_weight * T.sum(m.to(mu.dtype) * d * d) / mu.shape[0]
        for p, g in zip(self._actor_params, T.autograd.grad(actor_loss, self._actor_params)):
            p.grad = g
        if self.grad_sync_actor is not None:
            self.grad_sync_actor()
        if clip is not None and clip.actor is not None:
            T.nn.utils.clip_grad_norm_(self._actor_params, clip.actor)
        self.actor.optimizer.step()

        self.update_network_parameters()
        self.last_critic_loss, self.last_actor_loss = critic_loss.detach(), actor_loss.detach()

    def seed_td3_noise(self, seed):
        """Seed the generator of the torch path's target-smoothing noise (a loop seeds it with its own seed); its state is
        td3_noise_state() / set_td3_noise_state() for a checkpoint."""
        self._td3_gen.manual_seed((int(seed) ^ 0x7D3E) & (2 ** 63 - 1))

    def td3_noise_state(self):
        return self._td3_gen.get_state().clone()

    def set_td3_noise_state(self, state):
        self._td3_gen.set_state(state.cpu().to(T.uint8))

    def _learn_batch_td3(self, states, actions, rewards, states_, done, discount, eps=None, full=None):
        """One TD3 update in torch (the CPU path, and the twin the fused TD3 learner is tested against).
        eps [B]: the target-smoothing noise to use, in the actor's normalised action units (None: clip(target_noise * N(0, 1),
        +-noise_clip) from the agent's own generator).  full: None = every policy_delay-th update is a full one (actor step through
        the updated critic 1, then the soft update of all three targets); else this update is full or critic-only as told."""
        cfg = self.td3
        with T.no_grad():
            mu_t = self.target_actor.forward(states_)
            if eps is None:
                nrm = T.randn(mu_t.shape, generator=self._td3_gen, device=mu_t.device, dtype=mu_t.dtype)
                eps = (cfg.target_noise * nrm).clamp(-cfg.noise_clip, cfg.noise_clip)
            a2 = (mu_t + eps.to(mu_t).view_as(mu_t)).clamp(-1.0, 1.0)
            q_next = T.min(self.target_critic.forward(states_, a2), self.target_critic_2.forward(states_, a2))
            q_next = q_next.masked_fill(done.view(-1, 1), 0.0).view(-1)
            target = (rewards + discount * q_next).view(-1, 1)
        for net, params in ((self.critic, self._critic_params), (self.critic_2, self._critic_2_params)):
            loss = F.mse_loss(target, net.forward(states, actions))
            for p, g in zip(params, T.autograd.grad(loss, params)):
                p.grad = g
            net.optimizer.step()
            if net is self.critic:
                self.last_critic_loss = loss.detach()
        self.td3_updates += 1
        if full is None:
            full = self.td3_updates % cfg.policy_delay == 0
        if full:
            actor_loss = T.mean(-self.critic.forward(states, self.actor.forward(states)))
            for p, g in zip(self._actor_params, T.autograd.grad(actor_loss, self._actor_params)):
                p.grad = g
            self.actor.optimizer.step()
            self.update_network_parameters()
            self.last_actor_loss = actor_loss.detach()

    def update_network_parameters(self, tau=None):
        """theta' <- tau*theta + (1 - tau)*theta' over every named parameter (DDPG_agent.py:108-131)."""
        if tau is None:
            tau = self.tau
        with T.no_grad():
            pairs = ((self.critic, self.target_critic), (self.actor, self.target_actor))
            if getattr(self, "td3", None) is not None:
                pairs += ((self.critic_2, self.target_critic_2),)
            for net, target in pairs:
                src = [p.data for p in net.parameters()]
                dst = [p.data for p in target.parameters()]
                if tau == 1:
                    T._foreach_copy_(dst, src)
                else:
                    T._foreach_lerp_(dst, src, tau)     # theta' + tau*(theta - theta'): one multi-tensor kernel
