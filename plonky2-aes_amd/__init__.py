"""MI355X-native Plonky2 proving backend for the 0xPARC/plonky2-aes gadget circuits.

The directory name carries a hyphen (it mirrors the reference's name), so import it with
`importlib` -- see `load_package()` in `__graft_entry__.py` -- under the module name `plonky2_aes_amd`.
"""
from .api import (  # noqa: F401
    AesGcmTarget,
    CircuitBuilder,
    CircuitData,
    ECGFP5SecretKey,
    FAULT_KINDS,
    HASHERS,
    OP_KINDS,
    P2Error,
    PartialWitness,
    PoseidonEncryptTarget,
    ProveError,
    VERIFY_FINAL_POLY,
    VERIFY_FRI_FOLD,
    VERIFY_MERKLE_FRI,
    VERIFY_MERKLE_INITIAL,
    VERIFY_NON_CANONICAL,
    VERIFY_OK,
    VERIFY_POW,
    VERIFY_REASONS,
    VERIFY_SHAPE,
    VERIFY_VANISHING,
    VERIFY_ZETA_IN_SUBGROUP,
    VALUE_UNSET,
    WitnessFault,
    ecgfp5,
    host_witness,
    keccak_native,
    lib,
    lib_path,
    native,
    poseidon_native,
)
