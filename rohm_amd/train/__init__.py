"""RoHM's training loops on the native pieces: `python -m rohm_amd.train posenet|trajnet --config cfg.yaml`."""
from .loops import JsonlWriter, TrainLoopPoseNet, TrainLoopTrajNet  # noqa: F401
from .masks import (PoseMaskDecision, PoseMaskSchedule, ProxMaskBank, TrajMaskDecision, TrajMaskSchedule,  # noqa: F401
                    pack_prox_clips, train_cond, traj_window)
