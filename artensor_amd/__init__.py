"""artensor_amd: MI355X-native numerical contraction engine behind artensor's executor API.

Drop-in for the hot path of Fanerst/artensor:

    from artensor_amd import tensor_contraction, tensor_contraction_sparse   # executors
    from artensor_amd import contraction_scheme, contraction_scheme_sparse   # scheme compilers
    from artensor_amd import TensorNetworkSimulation, sliced_contraction     # slice loop, multi-GPU

    from artensor_amd import tensor_network_contraction, quantum_circuit_simulation   # one-call API

Planning (AbstractTensorNetwork / ContractionTree / find_order / GreedyOrderFinder, the circuit parser)
is not part of this package: the engine consumes the planner's products unchanged; the one-call API and
TensorNetworkSimulation.from_circuit_file / prepare_contraction forward the planning half to the
reference's front end (the installed `artensor` package, or `planner=`).
"""
from .contraction import (  # noqa: F401
    contract,
    contraction_scheme,
    contraction_scheme_sparse,
    einsum_eq_convert,
    precision,
    step_info,
    tensor_contraction,
    tensor_contraction_sparse,
)
from .fixtures import load_case, save_case  # noqa: F401
from .simulation import (  # noqa: F401
    SliceRunner,
    TensorNetworkSimulation,
    accumulate,
    apply_slice,
    partition_output,
    partitioned_contraction,
    plan_output_slabs,
    slab_contraction,
    quantum_circuit_simulation,
    rank_slices,
    slice_assignments,
    sliced_contraction,
    tensor_network_contraction,
)

from . import born  # noqa: F401
from .born import (  # noqa: F401
    fidelity,
    linear_xeb,
    marginal_probabilities,
    norm2,
    overlap,
    sample,
)
from . import rdm  # noqa: F401
from .rdm import (  # noqa: F401
    entanglement_entropy,
    entropy_of,
    expectation,
    purity,
    rdm_info,
    reduced_density_matrix,
    renyi_entropy,
)
from . import pauli  # noqa: F401
from .pauli import (  # noqa: F401
    PauliCircuit,
    PauliSumOperator,
    pauli_apply,
    pauli_apply_,
    pauli_apply_info,
    pauli_evolve_,
    pauli_evolve_info,
    pauli_expectation,
    pauli_info,
    pauli_ops,
    pauli_rotate,
    pauli_rotate_,
    pauli_sum_apply,
    pauli_sum_expectation,
    pauli_sum_variance,
    trotter_steps,
)
from . import adjoint  # noqa: F401
from .adjoint import (  # noqa: F401
    PauliPairCircuit,
    adjoint_gradient,
    pauli_adjoint_info,
    pauli_evolve_pair_,
)
from . import gates  # noqa: F401
from .gates import (  # noqa: F401
    GateCircuit,
    apply_gate_,
    apply_gates_,
    gate_circuit_info,
    gates_from_bonds,
    merge_gates,
    run_circuit,
)
from . import gate_adjoint  # noqa: F401
from .gate_adjoint import (  # noqa: F401
    GatePairCircuit,
    apply_gates_pair_,
    gate_adjoint_gradient,
    gate_adjoint_info,
    parametric_gate,
)
from . import wide_gates  # noqa: F401
from .wide_gates import (  # noqa: F401
    FusedCircuit,
    WideGate,
    apply_circuit_,
    apply_wide_gate_,
    fuse_gates,
    wide_gate_info,
)
from . import matrix_gates  # noqa: F401
from .matrix_gates import (  # noqa: F401
    BlockCircuit,
    MatrixGate,
    apply_blocks_,
    apply_matrix_gate_,
    fuse_gates_wide,
    matrix_gate_info,
)
from . import controlled  # noqa: F401
from .controlled import (  # noqa: F401
    ControlledGate,
    apply_controlled_gate_,
    controlled_gate_info,
    mcphase_,
    mcx_,
    mcz_,
    when,
)
from . import krylov  # noqa: F401
from .krylov import (  # noqa: F401
    KrylovResult,
    krylov_combine_,
    krylov_dots,
    krylov_evolve,
    krylov_info,
    lanczos,
    lanczos_ground_state,
)
from . import measure  # noqa: F401
from .measure import (  # noqa: F401
    apply_channel_,
    measure_,
    measure_info,
    postselect_,
    reset_,
)
from . import channel  # noqa: F401
from .channel import (  # noqa: F401
    Channel,
    ChannelOp,
    amplitude_damping,
    bit_flip,
    channel_,
    channel_info,
    channel_step_,
    depolarizing,
    pauli_channel,
    phase_damping,
    phase_flip,
)
from . import trajectories  # noqa: F401
from .trajectories import (  # noqa: F401
    BatchChannelOp,
    BatchConditionalGate,
    apply_conditional_gate_batch_,
    channel_batch_,
    collapse_batch_,
    conditional_gate_info,
    correct_batch_,
    measure_batch_,
    pauli_batch_info,
    pauli_expectation_batch,
    pauli_sum_expectation_batch,
    postselect_batch_,
    reset_batch_,
    sample_batch,
    sample_batch_flat,
    sample_batch_info,
    trajectory_info,
    trajectory_mean,
    trajectory_norms,
)
from . import diagonal  # noqa: F401
from .diagonal import (  # noqa: F401
    DiagonalOperator,
    diagonal_evolve_,
    diagonal_expectation,
    diagonal_info,
    diagonal_values,
    ising_terms,
    maxcut_terms,
    qaoa_gradient,
)
from . import layout  # noqa: F401
from .layout import (  # noqa: F401
    BitPermutation,
    bit_permutation_info,
    busiest_dims_order,
    permute_dims_,
    relayout_,
    reverse_qubits_,
    swap_dims_,
)
from .network import tn_contract  # noqa: F401
from .statevector import state_vec  # noqa: F401

__version__ = "0.1.0"
