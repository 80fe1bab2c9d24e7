"""The reference's four test scripts on the native pieces: `python -m rohm_amd.drivers amass_full|prox_egobody|posenet|trajnet`."""
from .results import (ResultWriter, TrajReport, amass_full_results, posenet_results, prox_egobody_results,  # noqa: F401
                      result_rows, step_schedule, traj_report, traj_report_lines, trajnet_results)
