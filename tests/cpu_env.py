"""The env stand-in of the CPU loop tests: what a VectorStepper asks of an env before its first step (no launch is ever made)."""
import numpy as np
import torch


class CpuEnv:
    observation_dim, n_envs, device, max_steer = 23, 4, torch.device("cpu"), float(np.float32(np.pi / 4))

    def observe(self, out=None):
        out.zero_()
        return out
