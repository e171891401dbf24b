"""Solver agreement check (reference: solvers/verification.py:12-44): SciPy, the cold lapjv and the
seeded lapjv must reach the same optimal cost.  Host glue over the solver wrappers."""
import numpy as np

from .scipy_solver import SciPySolver
from .lap_solver import LAPSolver, SeededLAPSolver


def verify_solver_correctness(C: np.ndarray, u_oracle: np.ndarray, v_oracle: np.ndarray,
                              tolerance: float = 1e-10) -> bool:
    """True when the three optimal costs agree within `tolerance`; prints and returns False on error."""
    try:
        scipy_solver = SciPySolver()
        lap_solver = LAPSolver()
        seeded_solver = SeededLAPSolver()

        _, _, scipy_cost = scipy_solver.solve(C)
        _, _, lap_cost = lap_solver.solve(C)
        _, _, seeded_cost = seeded_solver.solve(C, u_oracle, v_oracle)

        costs = [scipy_cost, lap_cost, seeded_cost]
        cost_range = max(costs) - min(costs)

        return cost_range < tolerance

    except Exception as e:
        print(f"Verification failed: {e}")
        return False
