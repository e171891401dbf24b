"""`solvers` -- same import surface as the reference's solvers package for the hot path
(/root/reference/solvers/__init__.py:27-58): solver wrappers, dual utilities, timing and the
input generators.  The LAP solves and the dense dual sweeps run on the MI355X through
liblapwarm_hip.so; SciPy is kept only as the external baseline the harness compares against.

Oracle duals (compute_oracle_duals, dual_from_matching_diff_constraints, make_feasible_duals)
run on the device too (csrc/oracle_duals.hip); their matching comes from lap.lapjv instead of
SciPy (solvers/dual_computation.py).

LAPMODSolver wraps the sparse solver (lap.lapmod_sparse, csrc/lapmod_sparse.hip).

Not provided (outside the hot path): logging helpers, seed_greedy_matching.
"""
from .scipy_solver import SciPySolver
from .lap_solver import LAPSolver, SeededLAPSolver
from .lapmod_solver import LAPMODSolver
from .warmstart_solver import WarmStartLAPSolver
from .timing import time_solver_rigorous
from .advanced_dual import (project_feasible, reduce_costs, check_dual_feasible, check_dual_and_match,
                            make_feasible_duals, project_feasible_many, reduce_costs_many,
                            check_dual_feasible_many)
from .dual_computation import compute_oracle_duals, dual_from_matching_diff_constraints
from .verification import verify_solver_correctness
from .seed_baselines import (seed_row_col_minima, seed_noisy_optimal, seed_row_col_minima_many,
                             seed_noisy_optimal_many)
from .generators import (
    generate_uniform_costs,
    generate_near_diagonal_costs,
    generate_sparse_costs,
    generate_metric_costs,
    generate_clustered_costs,
    generate_noisy_linear_costs,
    generate_worst_case_costs,
    generate_identity_like_costs,
    generate_hard_random_costs,
)

__all__ = [
    "SciPySolver", "LAPSolver", "SeededLAPSolver", "LAPMODSolver", "WarmStartLAPSolver", "time_solver_rigorous",
    "project_feasible", "reduce_costs", "check_dual_feasible", "check_dual_and_match", "make_feasible_duals",
    "compute_oracle_duals", "dual_from_matching_diff_constraints", "verify_solver_correctness",
    "seed_row_col_minima", "seed_noisy_optimal",
    "project_feasible_many", "reduce_costs_many", "check_dual_feasible_many",
    "seed_row_col_minima_many", "seed_noisy_optimal_many",
    "generate_uniform_costs", "generate_near_diagonal_costs", "generate_sparse_costs",
    "generate_metric_costs", "generate_clustered_costs", "generate_noisy_linear_costs",
    "generate_worst_case_costs", "generate_identity_like_costs", "generate_hard_random_costs",
]
