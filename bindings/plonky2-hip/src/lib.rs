//! `plonky2` as the 0xPARC/plonky2-aes gadget crates see it, backed by the MI355X-native
//! prover `libp2aes.so` through the C ABI of `include/p2aes.h`.
//!
//! Only what the reference calls is here -- `CircuitBuilder`, `Target`/`BoolTarget`, `PartialWitness` + `WitnessWrite`,
//! `CircuitConfig`, `CircuitData::{prove, verify, verify_compressed}`, proof compression, `GoldilocksField` with the `Field`/`Field64`/`Sample` methods used, the
//! `PoseidonHash` sponge -- under the module paths the reference imports them from.  Each item cites the call site it serves.
//! The module `pod2` at the bottom re-exports the handful of pod2 names the ecgfp5 / poseidon-cipher crates use.
//!
//! This file has not been compiled in this repository's image (no Rust toolchain); `ffi.rs` is generated from the header.
#![allow(clippy::new_without_default)]

pub mod ffi;

use std::ffi::CStr;
use std::marker::PhantomData;

fn last_error() -> anyhow::Error {
    let msg = unsafe { CStr::from_ptr(ffi::p2_last_error()) }.to_string_lossy().into_owned();
    anyhow::anyhow!(msg)
}

pub mod field {
    pub mod types {
        /// `plonky2::field::types::Field` -- the methods the reference calls (circuit_aes.rs:186,249; circuit_gcm.rs:339).
        pub trait Field: Copy + Eq + core::fmt::Debug {
            const ZERO: Self;
            const ONE: Self;
            const NEG_ONE: Self;
            fn from_canonical_u64(v: u64) -> Self;
            fn from_canonical_u8(v: u8) -> Self { Self::from_canonical_u64(v as u64) }
            fn to_canonical_u64(&self) -> u64;
        }
        /// `Field64::ORDER` (ecgfp5/src/lib.rs:56).
        pub trait Field64: Field {
            const ORDER: u64;
        }
        /// `Sample::rand` (poseidon-cipher/src/lib.rs:143-144): uniform field element from the OS RNG.
        pub trait Sample: Sized {
            fn rand() -> Self;
        }
    }
    pub mod goldilocks_field {
        use super::types::{Field, Field64, Sample};
        /// Canonical representative in [0, p), p = 2^64 - 2^32 + 1.
        #[derive(Copy, Clone, Debug, Default, Eq, PartialEq, Hash)]
        pub struct GoldilocksField(pub u64);
        impl Field for GoldilocksField {
            const ZERO: Self = GoldilocksField(0);
            const ONE: Self = GoldilocksField(1);
            const NEG_ONE: Self = GoldilocksField(<Self as Field64>::ORDER - 1);
            fn from_canonical_u64(v: u64) -> Self { debug_assert!(v < <Self as Field64>::ORDER); GoldilocksField(v) }
            fn to_canonical_u64(&self) -> u64 { self.0 }
        }
        impl Field64 for GoldilocksField {
            const ORDER: u64 = 0xFFFF_FFFF_0000_0001;
        }
        impl Sample for GoldilocksField {
            fn rand() -> Self {
                use rand::RngCore;
                loop {
                    let v = rand::rngs::OsRng.next_u64();
                    if v < <Self as Field64>::ORDER { return GoldilocksField(v); }
                }
            }
        }
    }
    pub mod extension {
        /// Marker only: the backend fixes D = 2 (`standard_recursion_config`), the gadgets never touch extension elements.
        pub trait Extendable<const D: usize> {}
        impl Extendable<2> for super::goldilocks_field::GoldilocksField {}
        pub mod quintic {
            /// GF(p^5) element as its five coefficients (ecgfp5/src/lib.rs:64-69: `from_basefield_array`).
            #[derive(Copy, Clone, Debug, Eq, PartialEq)]
            pub struct QuinticExtension<F>(pub [F; 5]);
            impl<F: Copy> QuinticExtension<F> {
                pub fn from_basefield_array(a: [F; 5]) -> Self { QuinticExtension(a) }
            }
        }
    }
}

pub mod hash {
    pub mod hash_types {
        pub trait RichField: crate::field::types::Field64 {}
        impl RichField for crate::field::goldilocks_field::GoldilocksField {}
        use crate::iop::target::Target;
        /// `HashOut<F>`: four field elements.
        pub type HashOut = [crate::field::goldilocks_field::GoldilocksField; 4];
        #[derive(Copy, Clone, Debug)]
        pub struct HashOutTarget { pub elements: [Target; 4] }
        #[derive(Clone, Debug)]
        pub struct MerkleCapTarget(pub Vec<HashOutTarget>);
    }
    pub mod poseidon {
        /// Marker for `builder.hash_n_to_m_no_pad::<PoseidonHash>` (poseidon-cipher/src/circuit.rs:123).
        pub struct PoseidonHash;
        pub struct PoseidonPermutation<F>(core::marker::PhantomData<F>);
    }
    pub mod merkle_proofs {
        use super::hash_types::{HashOut, HashOutTarget};
        use crate::field::goldilocks_field::GoldilocksField as F;
        #[derive(Clone, Debug)]
        pub struct MerkleProof { pub siblings: Vec<HashOut> }
        #[derive(Clone, Debug)]
        pub struct MerkleProofTarget { pub siblings: Vec<HashOutTarget> }
        /// `verify_merkle_proof_to_cap::<F, PoseidonHash>` on the host (p2_native_merkle_verify).
        pub fn verify_merkle_proof_to_cap(leaf_data: &[F], leaf_index: usize, merkle_cap: &[HashOut], proof: &MerkleProof) -> Result<(), String> {
            let leaf: Vec<u64> = leaf_data.iter().map(|x| x.0).collect();
            let cap: Vec<u64> = merkle_cap.iter().flat_map(|h| h.iter().map(|x| x.0)).collect();
            let sib: Vec<u64> = proof.siblings.iter().flat_map(|h| h.iter().map(|x| x.0)).collect();
            let mut status: std::os::raw::c_int = -1;
            let rc = unsafe { crate::ffi::p2_native_merkle_verify(leaf.as_ptr(), leaf.len(), leaf_index, sib.as_ptr(), proof.siblings.len(), cap.as_ptr(), merkle_cap.len().trailing_zeros() as std::os::raw::c_int, &mut status) };
            if rc != crate::ffi::P2_OK { return Err(crate::last_error()); }
            if status == 0 { Ok(()) } else { Err("Invalid Merkle proof.".into()) }
        }
    }
    pub mod merkle_tree {
        use super::hash_types::HashOut;
        use super::merkle_proofs::MerkleProof;
        use crate::field::goldilocks_field::GoldilocksField as F;
        /// `MerkleTree::<F, PoseidonHash>::new(leaves, cap_height)`: built and kept on HIP device 0 (p2_merkle_tree_new).
        pub struct MerkleTree { h: *mut std::os::raw::c_void, depth: usize, pub cap: Vec<HashOut> }
        impl Drop for MerkleTree {
            fn drop(&mut self) { unsafe { crate::ffi::p2_merkle_tree_free(self.h) } }
        }
        impl MerkleTree {
            pub fn new(leaves: Vec<Vec<F>>, cap_height: usize) -> Self {
                let leaf_len = leaves.first().map_or(0, |l| l.len());
                assert!(leaves.iter().all(|l| l.len() == leaf_len), "leaves of unequal length");
                let flat: Vec<u64> = leaves.iter().flat_map(|l| l.iter().map(|x| x.0)).collect();
                let mut h: *mut std::os::raw::c_void = core::ptr::null_mut();
                let rc = unsafe { crate::ffi::p2_merkle_tree_new(flat.as_ptr(), leaves.len(), leaf_len, cap_height as std::os::raw::c_int, 0, &mut h) };
                assert!(rc == crate::ffi::P2_OK, "{}", crate::last_error());
                let mut cap = vec![0u64; 4 << cap_height];
                let rc = unsafe { crate::ffi::p2_merkle_tree_cap(h, cap.as_mut_ptr(), cap.len()) };
                assert!(rc == crate::ffi::P2_OK, "{}", crate::last_error());
                let depth = leaves.len().trailing_zeros() as usize - cap_height;
                MerkleTree { h, depth, cap: cap.chunks(4).map(|c| core::array::from_fn(|i| F(c[i]))).collect() }
            }
            pub fn prove(&self, leaf_index: usize) -> MerkleProof {
                let idx = [leaf_index as u64];
                let mut out = vec![0u64; 4 * self.depth.max(1)];
                let rc = unsafe { crate::ffi::p2_merkle_tree_prove_batch(self.h, idx.as_ptr(), 1, out.as_mut_ptr()) };
                assert!(rc == crate::ffi::P2_OK, "{}", crate::last_error());
                MerkleProof { siblings: out[..4 * self.depth].chunks(4).map(|c| core::array::from_fn(|i| F(c[i]))).collect() }
            }
        }
    }
    pub mod hashing {
        use crate::field::goldilocks_field::GoldilocksField as F;
        /// Native `hash_n_to_m_no_pad::<F, PoseidonPermutation<_>>` (poseidon-cipher/src/lib.rs:116).
        pub fn hash_n_to_m_no_pad(inputs: &[F], m: usize) -> Vec<F> {
            let inp: Vec<u64> = inputs.iter().map(|x| x.0).collect();
            let mut out = vec![0u64; m];
            unsafe { crate::ffi::p2_native_hash_n_to_m_no_pad(inp.as_ptr(), inp.len(), out.as_mut_ptr(), m) };
            out.into_iter().map(F).collect()
        }
    }
}

pub mod iop {
    pub mod target {
        /// Opaque handle of the backend: a virtual target index, or bit 63 | row << 8 | column for a routed wire.
        #[derive(Copy, Clone, Debug, Eq, PartialEq, Hash)]
        pub struct Target(pub u64);
        #[derive(Copy, Clone, Debug, Eq, PartialEq, Hash)]
        pub struct BoolTarget { pub target: Target }
        impl BoolTarget {
            pub fn new_unsafe(target: Target) -> Self { BoolTarget { target } }   // circuit_gcm.rs:424
        }
    }
    pub mod witness {
        use super::target::Target;
        use crate::field::types::Field;
        use core::marker::PhantomData;
        /// `PartialWitness::new` + `set_target` (circuit_aes.rs:283,401): the sparse input map handed to `prove`.
        pub struct PartialWitness<F> {
            pub(crate) targets: Vec<u64>,
            pub(crate) values: Vec<u64>,
            _f: PhantomData<F>,
        }
        impl<F> PartialWitness<F> {
            pub fn new() -> Self { PartialWitness { targets: Vec::new(), values: Vec::new(), _f: PhantomData } }
        }
        pub trait WitnessWrite<F: Field> {
            fn set_target(&mut self, target: Target, value: F) -> anyhow::Result<()>;
            fn set_target_arr(&mut self, targets: &[Target], values: &[F]) -> anyhow::Result<()> {
                anyhow::ensure!(targets.len() == values.len(), "set_target_arr: length mismatch");
                for (t, v) in targets.iter().zip(values) { self.set_target(*t, *v)?; }
                Ok(())
            }
        }
        /// What `CircuitData::generate_partial_witness` returns: the value the witness run gave every virtual target of the
        /// circuit (upstream's `PartitionWitness`, read with `get_target`).  Routed wires are read with
        /// `CircuitData::generate_witness_targets`.
        pub struct Witness<F> {
            pub(crate) values: Vec<u64>,   // by virtual target index; u64::MAX = the run did not determine it
            pub(crate) _f: PhantomData<F>,
        }
        impl<F: Field> Witness<F> {
            /// `None` for a routed wire, a target of another circuit, or a target the run did not determine.
            pub fn try_get_target(&self, target: Target) -> Option<F> {
                match self.values.get(usize::try_from(target.0).ok()?) {
                    Some(&v) if v != crate::ffi::P2_VALUE_UNSET => Some(F::from_canonical_u64(v)),
                    _ => None,
                }
            }
            /// `Witness::get_target`; panics where upstream does (the target has no value).
            pub fn get_target(&self, target: Target) -> F {
                self.try_get_target(target).unwrap_or_else(|| panic!("target {:?} has no value in this witness", target))
            }
            pub fn get_targets(&self, targets: &[Target]) -> Vec<F> { targets.iter().map(|t| self.get_target(*t)).collect() }
        }
        impl<F: Field> WitnessWrite<F> for PartialWitness<F> {
            /// Setting a target twice is fine when the values agree and an error otherwise, as in plonky2.
            fn set_target(&mut self, target: Target, value: F) -> anyhow::Result<()> {
                let v = value.to_canonical_u64();
                if let Some(i) = self.targets.iter().position(|t| *t == target.0) {
                    anyhow::ensure!(self.values[i] == v, "target {:?} set twice with different values", target);
                    return Ok(());
                }
                self.targets.push(target.0);
                self.values.push(v);
                Ok(())
            }
        }
    }
}

pub mod plonk {
    pub mod config {
        /// The hash configuration `build::<C>()` compiles a circuit for (upstream `GenericConfig`'s `Hasher`).
        pub trait GenericConfig { const HASHER: std::os::raw::c_int; }
        /// `PoseidonGoldilocksConfig`: Poseidon Merkle trees, challenger and circuit digest.
        pub struct PoseidonGoldilocksConfig;
        impl GenericConfig for PoseidonGoldilocksConfig { const HASHER: std::os::raw::c_int = crate::ffi::P2_HASHER_POSEIDON; }
        /// `KeccakGoldilocksConfig`: Merkle trees and circuit digest by Keccak-256 truncated to 25 bytes (`KeccakHash<25>`), the
        /// challenger still Poseidon -- the configuration for proofs that are not verified inside another circuit.
        pub struct KeccakGoldilocksConfig;
        impl GenericConfig for KeccakGoldilocksConfig { const HASHER: std::os::raw::c_int = crate::ffi::P2_HASHER_KECCAK; }
    }
    pub mod circuit_data {
        use crate::field::types::Field;
        use crate::iop::target::Target;
        use crate::iop::witness::{PartialWitness, Witness};
        use crate::{ffi, last_error};
        use core::marker::PhantomData;

        /// `CircuitConfig::standard_recursion_config()` / `standard_recursion_zk_config()` (circuit_gcm.rs:757,
        /// examples/aes_gcm_128.rs:36) -- the two configurations the reference instantiates.
        #[derive(Clone, Copy, Debug)]
        pub struct CircuitConfig { pub zero_knowledge: bool }
        impl CircuitConfig {
            pub fn standard_recursion_config() -> Self { CircuitConfig { zero_knowledge: false } }
            pub fn standard_recursion_zk_config() -> Self { CircuitConfig { zero_knowledge: true } }
        }

        /// Serialised proof exactly as the device writes it ("Proof layout"), and the values of the circuit's
        /// public inputs in registration order, parsed from the proof's trailer (empty for a circuit without any).
        pub struct ProofWithPublicInputs<F, C, const D: usize> {
            pub bytes: Vec<u8>,
            pub public_inputs: Vec<F>,
            pub(crate) _p: PhantomData<(F, C)>,
        }
        impl<F, C, const D: usize> ProofWithPublicInputs<F, C, D> {
            pub fn to_bytes(&self) -> Vec<u8> { self.bytes.clone() }
        }
        impl<F: Field, C, const D: usize> ProofWithPublicInputs<F, C, D> {
            /// `ProofWithPublicInputs::compress`.  Upstream takes `(circuit_digest, common_data)`; here
            /// the circuit data that holds both.
            pub fn compress(self, data: &CircuitData<F, C, D>) -> anyhow::Result<CompressedProofWithPublicInputs<F, C, D>> {
                let bytes = data.convert(ffi::p2_proof_compress, &self.bytes)?;
                Ok(CompressedProofWithPublicInputs { bytes, public_inputs: self.public_inputs, _p: PhantomData })
            }
        }

        /// A compressed proof: the full proof's caps, openings and tail, its query indices, and each Merkle sibling and FRI
        /// evaluation that the indices do not already imply.
        pub struct CompressedProofWithPublicInputs<F, C, const D: usize> {
            pub bytes: Vec<u8>,
            pub public_inputs: Vec<F>,
            pub(crate) _p: PhantomData<(F, C)>,
        }
        impl<F: Field, C, const D: usize> CompressedProofWithPublicInputs<F, C, D> {
            pub fn to_bytes(&self) -> Vec<u8> { self.bytes.clone() }
            /// `CompressedProofWithPublicInputs::decompress`; upstream's `(circuit_digest, common_data)` as in `compress`.
            pub fn decompress(self, data: &CircuitData<F, C, D>) -> anyhow::Result<ProofWithPublicInputs<F, C, D>> {
                let bytes = data.convert(ffi::p2_proof_decompress, &self.bytes)?;
                Ok(ProofWithPublicInputs { bytes, public_inputs: self.public_inputs, _p: PhantomData })
            }
        }

        /// Result of `builder.build::<PoseidonGoldilocksConfig>()`: the compiled circuit, resident on one MI355X.
        pub struct CircuitData<F, C, const D: usize> {
            pub(crate) handle: *mut ffi::P2Circuit,
            pub(crate) blob: Vec<u8>,
            pub(crate) verifier_data: Vec<u64>,
            pub(crate) num_public_inputs: usize,   // read once at build: every proof of the circuit has this many
            pub(crate) _p: PhantomData<(F, C)>,
        }
        // `prove(&self)` takes a shared reference and the handle serialises its own enqueues (include/p2aes.h).
        unsafe impl<F, C, const D: usize> Send for CircuitData<F, C, D> {}
        unsafe impl<F, C, const D: usize> Sync for CircuitData<F, C, D> {}
        impl<F, C, const D: usize> Drop for CircuitData<F, C, D> {
            fn drop(&mut self) { unsafe { ffi::p2_circuit_free(self.handle) } }
        }
        impl<F: Field, C, const D: usize> CircuitData<F, C, D> {
            /// circuit_gcm.rs:781 and the 19 other `.prove(` sites.  `Err` when witness generation
            /// fails -- the behaviour circuit_aes.rs:403-405 pins.
            pub fn prove(&self, pw: PartialWitness<F>) -> anyhow::Result<ProofWithPublicInputs<F, C, D>> {
                let mut proofs = self.prove_batch(&[pw])?;
                proofs.pop().unwrap()
            }
            /// Many witnesses of one circuit in one call -- the shape of ecgfp5/src/elgamal/circuit.rs:76-96 -- which is
            /// what fills the GPU.  One `Result` per witness.
            pub fn prove_batch(&self, pws: &[PartialWitness<F>]) -> anyhow::Result<Vec<anyhow::Result<ProofWithPublicInputs<F, C, D>>>> {
                let pb = unsafe { ffi::p2_circuit_proof_bytes(self.handle) };
                let asg: Vec<ffi::P2Assignment> = pws.iter()
                    .map(|pw| ffi::P2Assignment { targets: pw.targets.as_ptr(), values: pw.values.as_ptr(), count: pw.targets.len() })
                    .collect();
                let mut bytes = vec![0u8; pb * pws.len()];
                let mut status = vec![0 as std::os::raw::c_int; pws.len()];
                let rc = unsafe { ffi::p2_prove_batch(self.handle, pws.len(), asg.as_ptr(), bytes.as_mut_ptr(), status.as_mut_ptr()) };
                if rc != ffi::P2_OK { return Err(last_error()); }
                Ok(status.iter().enumerate().map(|(i, st)| match *st {
                    0 => {
                        let proof = bytes[i * pb..(i + 1) * pb].to_vec();
                        let public_inputs = self.parse_public_inputs(&proof)?;
                        Ok(ProofWithPublicInputs { bytes: proof, public_inputs, _p: PhantomData })
                    }
                    1 => Err(anyhow::anyhow!("witness generation failed: conflicting value or lookup input not in table")),
                    2 => Err(anyhow::anyhow!("witness generation failed: a generator never ran (an input target was not set)")),
                    3 => Err(anyhow::anyhow!("Opening point is in the subgroup.")),
                    s => Err(anyhow::anyhow!("prove failed with status {s}")),
                }).collect())
            }
            /// Witness generation on the GPU without proving (upstream `generate_partial_witness`): set the inputs, read what the
            /// circuit computed with `Witness::get_target`.  `Err` carries the explained fault (`p2_witness_explain`): which
            /// target, which entry of `pw`, what was computed and what was found.
            pub fn generate_partial_witness(&self, pw: PartialWitness<F>) -> anyhow::Result<Witness<F>> {
                let mut info = ffi::P2CircuitInfo::default();
                let rc = unsafe { ffi::p2_blob_info(self.blob.as_ptr(), self.blob.len(), &mut info) };
                if rc != ffi::P2_OK { return Err(last_error()); }
                let all: Vec<Target> = (0..info.num_virtual_targets as u64).map(Target).collect();
                let values = self.generate_witness_raw(&pw, &all)?;
                Ok(Witness { values, _f: PhantomData })
            }
            /// The same for a chosen list of targets, routed wires included; one value per target, in order.
            pub fn generate_witness_targets(&self, pw: PartialWitness<F>, targets: &[Target]) -> anyhow::Result<Vec<F>> {
                let values = self.generate_witness_raw(&pw, targets)?;
                values.iter().zip(targets).map(|(&v, t)| {
                    anyhow::ensure!(v != ffi::P2_VALUE_UNSET, "target {:?} has no value in this witness", t);
                    Ok(F::from_canonical_u64(v))
                }).collect()
            }
            fn generate_witness_raw(&self, pw: &PartialWitness<F>, targets: &[Target]) -> anyhow::Result<Vec<u64>> {
                let asg = ffi::P2Assignment { targets: pw.targets.as_ptr(), values: pw.values.as_ptr(), count: pw.targets.len() };
                let outs: Vec<u64> = targets.iter().map(|t| t.0).collect();
                let mut values = vec![0u64; outs.len()];
                let mut status: std::os::raw::c_int = 0;
                let rc = unsafe { ffi::p2_witness_batch(self.handle, 1, &asg, outs.as_ptr(), outs.len(), values.as_mut_ptr(), &mut status) };
                if rc != ffi::P2_OK { return Err(last_error()); }
                if status == 0 { return Ok(values); }
                let mut fault = ffi::P2WitnessFault::default();
                let rc = unsafe { ffi::p2_witness_explain(self.handle, &asg, &mut status, &mut fault as *mut ffi::P2WitnessFault as *mut std::os::raw::c_void) };
                if rc != ffi::P2_OK { return Err(last_error()); }
                let kind = ffi::P2_FAULT_KINDS.get(fault.kind as usize).copied().unwrap_or("UNKNOWN");
                Err(anyhow::anyhow!("witness generation failed ({kind}): target {:#x}, entry {} of the witness, gate row {}, computed {}, found {}",
                                    fault.target, fault.input_index, fault.gate_row as i32, fault.computed, fault.found))
            }
            /// The public-input trailer of a proof of this circuit: u64 k || k values, the last 8 (k + 1) bytes (none for k = 0).
            /// Reads those bytes only, so it costs O(k) per proof of a batch.
            fn parse_public_inputs(&self, proof: &[u8]) -> anyhow::Result<Vec<F>> {
                let k = self.num_public_inputs;
                if k == 0 { return Ok(Vec::new()); }
                anyhow::ensure!(proof.len() >= 8 * (k + 1), "proof shorter than its public-input trailer");
                let t = &proof[proof.len() - 8 * (k + 1)..];
                let word = |i: usize| u64::from_le_bytes(t[8 * i..8 * i + 8].try_into().unwrap());
                anyhow::ensure!(word(0) == k as u64, "wrong number of public inputs");
                Ok((1..=k).map(|i| F::from_canonical_u64(word(i))).collect())
            }
            /// circuit_gcm.rs:782 (19 sites).
            pub fn verify(&self, proof: ProofWithPublicInputs<F, C, D>) -> anyhow::Result<()> {
                let rc = unsafe {
                    ffi::p2_verify(self.blob.as_ptr(), self.blob.len(), self.verifier_data.as_ptr(), self.verifier_data.len(),
                                   proof.bytes.as_ptr(), proof.bytes.len())
                };
                if rc != ffi::P2_OK { return Err(last_error()); }
                Ok(())
            }
            /// `CircuitData::verify_compressed`: verify of the decompressed proof, behind the checks of decompression.
            pub fn verify_compressed(&self, compressed_proof_with_pis: CompressedProofWithPublicInputs<F, C, D>) -> anyhow::Result<()> {
                let p = &compressed_proof_with_pis.bytes;
                let rc = unsafe {
                    ffi::p2_verify_compressed(self.blob.as_ptr(), self.blob.len(), self.verifier_data.as_ptr(), self.verifier_data.len(),
                                              p.as_ptr(), p.len())
                };
                if rc != ffi::P2_OK { return Err(last_error()); }
                Ok(())
            }
            /// p2_proof_compress / p2_proof_decompress into a buffer of the full proof size (never too small).
            pub(crate) fn convert(&self, f: unsafe extern "C" fn(*const u8, usize, *const u64, usize, *const u8, usize, *mut u8, usize, *mut usize) -> std::os::raw::c_int,
                                  input: &[u8]) -> anyhow::Result<Vec<u8>> {
                let pb = unsafe { ffi::p2_circuit_proof_bytes(self.handle) };
                let mut out = vec![0u8; pb];
                let mut n = 0usize;
                let rc = unsafe {
                    f(self.blob.as_ptr(), self.blob.len(), self.verifier_data.as_ptr(), self.verifier_data.len(), input.as_ptr(), input.len(),
                      out.as_mut_ptr(), out.len(), &mut n)
                };
                if rc != ffi::P2_OK { return Err(last_error()); }
                out.truncate(n);
                Ok(out)
            }
        }
    }
    pub mod circuit_builder {
        use super::circuit_data::{CircuitConfig, CircuitData};
        use crate::field::types::Field;
        use crate::hash::hash_types::{HashOutTarget, MerkleCapTarget};
        use crate::hash::merkle_proofs::MerkleProofTarget;
        use crate::iop::target::{BoolTarget, Target};
        use crate::{ffi, last_error};
        use core::marker::PhantomData;
        use std::sync::Arc;

        /// `CircuitBuilder::<F, D>::new(config)` and the methods of SURVEY.md A.1, one FFI call each.
        pub struct CircuitBuilder<F, const D: usize> { pub(crate) h: *mut ffi::P2Builder, _f: PhantomData<F> }
        impl<F, const D: usize> Drop for CircuitBuilder<F, D> {
            fn drop(&mut self) { unsafe { ffi::p2_builder_free(self.h) } }
        }
        impl<F: Field, const D: usize> CircuitBuilder<F, D> {
            pub fn new(config: CircuitConfig) -> Self {
                let h = unsafe { if config.zero_knowledge { ffi::p2_builder_new_zk() } else { ffi::p2_builder_new() } };
                CircuitBuilder { h, _f: PhantomData }
            }
            pub fn add_virtual_target(&mut self) -> Target { Target(unsafe { ffi::p2_builder_add_virtual_target(self.h) }) }   // circuit_aes.rs:178
            pub fn add_virtual_target_arr<const N: usize>(&mut self) -> [Target; N] { core::array::from_fn(|_| self.add_virtual_target()) }
            pub fn constant(&mut self, c: F) -> Target { Target(unsafe { ffi::p2_builder_constant(self.h, c.to_canonical_u64()) }) }   // :186
            pub fn zero(&mut self) -> Target { Target(unsafe { ffi::p2_builder_zero(self.h) }) }
            pub fn one(&mut self) -> Target { Target(unsafe { ffi::p2_builder_one(self.h) }) }
            /// c * x + y (circuit_aes.rs:249,356; circuit_gcm.rs:339,342,423)
            pub fn mul_const_add(&mut self, c: F, x: Target, y: Target) -> Target {
                Target(unsafe { ffi::p2_builder_mul_const_add(self.h, c.to_canonical_u64(), x.0, y.0) })
            }
            pub fn add(&mut self, x: Target, y: Target) -> Target { Target(unsafe { ffi::p2_builder_add(self.h, x.0, y.0) }) }   // circuit_gcm.rs:361
            pub fn sub(&mut self, x: Target, y: Target) -> Target { Target(unsafe { ffi::p2_builder_sub(self.h, x.0, y.0) }) }
            pub fn mul(&mut self, x: Target, y: Target) -> Target { Target(unsafe { ffi::p2_builder_mul(self.h, x.0, y.0) }) }   // :363
            pub fn is_equal(&mut self, x: Target, y: Target) -> BoolTarget {                                                      // :362
                BoolTarget::new_unsafe(Target(unsafe { ffi::p2_builder_is_equal(self.h, x.0, y.0) }))
            }
            pub fn select(&mut self, b: BoolTarget, x: Target, y: Target) -> Target {                                             // :314,323,364
                Target(unsafe { ffi::p2_builder_select(self.h, b.target.0, x.0, y.0) })
            }
            pub fn connect(&mut self, x: Target, y: Target) { unsafe { ffi::p2_builder_connect(self.h, x.0, y.0) } }              // :163
            /// `register_public_input`: every proof carries the target's value (ProofWithPublicInputs::public_inputs).
            pub fn register_public_input(&mut self, t: Target) {
                let rc = unsafe { ffi::p2_builder_register_public_input(self.h, t.0) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            pub fn register_public_inputs(&mut self, ts: &[Target]) { for &t in ts { self.register_public_input(t) } }
            /// circuit_aes.rs:300,317,334; circuit_gcm.rs:396,415.  `(u16, u16)` is two adjacent u16 in memory.
            pub fn add_lookup_table_from_pairs(&mut self, table: Arc<Vec<(u16, u16)>>) -> usize {
                // (u16, u16) has no guaranteed layout (repr(Rust)): flatten to the [in, out, in, out, ...] array the C ABI reads
                let flat: Vec<u16> = table.iter().flat_map(|&(a, b)| [a, b]).collect();
                let i = unsafe { ffi::p2_builder_add_lookup_table_from_pairs(self.h, flat.as_ptr(), table.len()) };
                assert!(i != usize::MAX, "{}", last_error());   // an empty table (upstream panics too)
                i
            }
            /// circuit_aes.rs:182,193,250,357; circuit_gcm.rs:403,424.
            pub fn add_lookup_from_index(&mut self, looking_in: Target, lut_index: usize) -> Target {
                let t = unsafe { ffi::p2_builder_add_lookup_from_index(self.h, looking_in.0, lut_index) };
                assert!(t != u64::MAX, "{}", last_error());
                Target(t)
            }
            /// `hash_n_to_m_no_pad::<PoseidonHash>` (poseidon-cipher/src/circuit.rs:123, hashed_elgamal/circuit.rs:42).
            pub fn hash_n_to_m_no_pad<H>(&mut self, inputs: Vec<Target>, m: usize) -> Vec<Target> {
                let inp: Vec<u64> = inputs.iter().map(|t| t.0).collect();
                let mut out = vec![0u64; m];
                let rc = unsafe { ffi::p2_builder_hash_n_to_m_no_pad(self.h, inp.as_ptr(), inp.len(), out.as_mut_ptr(), m) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                out.into_iter().map(Target).collect()
            }
            /// `assert_bool`: t * t - t = 0.
            pub fn assert_bool(&mut self, b: BoolTarget) {
                let rc = unsafe { ffi::p2_builder_assert_bool(self.h, b.target.0) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            /// `le_sum` of 1 to 64 little-endian bits.  Unlike upstream's, with exactly 64 bits it also refuses the spelling
            /// of value + p: the result always denotes the integer the bits spell.
            pub fn le_sum(&mut self, bits: impl Iterator<Item = impl std::borrow::Borrow<BoolTarget>>) -> Target {
                let inp: Vec<u64> = bits.map(|b| b.borrow().target.0).collect();
                let mut out = 0u64;
                let rc = unsafe { ffi::p2_builder_le_sum(self.h, inp.as_ptr(), inp.len(), &mut out) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                Target(out)
            }
            /// `split_le`: the num_bits (1 to 64) little-endian bits of x; no witness exists if x >= 2^num_bits.
            pub fn split_le(&mut self, x: Target, num_bits: usize) -> Vec<BoolTarget> {
                let mut out = vec![0u64; num_bits.clamp(1, 64)];
                let rc = unsafe { ffi::p2_builder_split_le(self.h, x.0, num_bits, out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                out.into_iter().map(|t| BoolTarget::new_unsafe(Target(t))).collect()
            }
            /// `range_check`: x < 2^n_log, n_log 1 to 63.
            pub fn range_check(&mut self, x: Target, n_log: usize) {
                let rc = unsafe { ffi::p2_builder_range_check(self.h, x.0, n_log) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            /// `permute_swapped::<PoseidonHash>`: one PoseidonGate row; the first two quarters of `inputs` are exchanged where swap = 1.
            pub fn permute_swapped(&mut self, inputs: [Target; 12], swap: BoolTarget) -> [Target; 12] {
                let inp: [u64; 12] = core::array::from_fn(|i| inputs[i].0);
                let mut out = [0u64; 12];
                let rc = unsafe { ffi::p2_builder_permute_swapped(self.h, inp.as_ptr(), swap.target.0, out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                out.map(Target)
            }
            /// `hash_or_noop::<PoseidonHash>`: up to four targets zero-padded as they are, more hashed.
            pub fn hash_or_noop<H>(&mut self, inputs: Vec<Target>) -> HashOutTarget {
                let inp: Vec<u64> = inputs.iter().map(|t| t.0).collect();
                let mut out = [0u64; 4];
                let rc = unsafe { ffi::p2_builder_hash_or_noop(self.h, inp.as_ptr(), inp.len(), out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                HashOutTarget { elements: out.map(Target) }
            }
            pub fn add_virtual_hash(&mut self) -> HashOutTarget {
                let mut out = [0u64; 4];
                let rc = unsafe { ffi::p2_builder_add_virtual_hash(self.h, out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                HashOutTarget { elements: out.map(Target) }
            }
            pub fn add_virtual_cap(&mut self, cap_height: usize) -> MerkleCapTarget {
                assert!(cap_height <= 16, "add_virtual_cap: cap_height must be 0 to 16");
                let mut out = vec![0u64; 4 << cap_height];
                let rc = unsafe { ffi::p2_builder_add_virtual_cap(self.h, cap_height as std::os::raw::c_int, out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                MerkleCapTarget(out.chunks(4).map(|c| HashOutTarget { elements: core::array::from_fn(|i| Target(c[i])) }).collect())
            }
            pub fn connect_hashes(&mut self, x: HashOutTarget, y: HashOutTarget) {
                let (a, b): ([u64; 4], [u64; 4]) = (x.elements.map(|t| t.0), y.elements.map(|t| t.0));
                let rc = unsafe { ffi::p2_builder_connect_hashes(self.h, a.as_ptr(), b.as_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            /// `verify_merkle_proof_to_cap::<PoseidonHash>`: leaf_data is the leaf at the index the little-endian bits spell.  The
            /// cap entry is chosen by a mux tree of `select` (upstream: a RandomAccessGate); the cap-index bits are made boolean here.
            pub fn verify_merkle_proof_to_cap<H>(&mut self, leaf_data: Vec<Target>, leaf_index_bits: &[BoolTarget], merkle_cap: &MerkleCapTarget, proof: &MerkleProofTarget) {
                let leaf: Vec<u64> = leaf_data.iter().map(|t| t.0).collect();
                let bits: Vec<u64> = leaf_index_bits.iter().map(|b| b.target.0).collect();
                let cap: Vec<u64> = merkle_cap.0.iter().flat_map(|h| h.elements.iter().map(|t| t.0)).collect();
                let sib: Vec<u64> = proof.siblings.iter().flat_map(|h| h.elements.iter().map(|t| t.0)).collect();
                let h = merkle_cap.0.len().trailing_zeros() as std::os::raw::c_int;
                assert!(merkle_cap.0.len().is_power_of_two(), "the cap must hold a power of two of hashes");
                let rc = unsafe { ffi::p2_builder_verify_merkle_proof_to_cap(self.h, leaf.as_ptr(), leaf.len(), bits.as_ptr(), bits.len(), cap.as_ptr(), h, sib.as_ptr(), proof.siblings.len()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            pub fn verify_merkle_proof<H>(&mut self, leaf_data: Vec<Target>, leaf_index_bits: &[BoolTarget], merkle_root: HashOutTarget, proof: &MerkleProofTarget) {
                self.verify_merkle_proof_to_cap::<H>(leaf_data, leaf_index_bits, &MerkleCapTarget(vec![merkle_root]), proof)
            }
            /// Not upstream's: the tree with cap `old_cap` holds `old_leaf` at the index; returns the cap of the same tree with
            /// `new_leaf` there.  Two walks over the same siblings and bits; the siblings are one item of `p2_merkle_tree_update`'s trace.
            pub fn merkle_update_to_cap<H>(&mut self, old_leaf: Vec<Target>, new_leaf: Vec<Target>, leaf_index_bits: &[BoolTarget], old_cap: &MerkleCapTarget, proof: &MerkleProofTarget) -> MerkleCapTarget {
                assert!(old_cap.0.len().is_power_of_two(), "the cap must hold a power of two of hashes");
                assert!(old_leaf.len() == new_leaf.len(), "the old and the new leaf must have one length");
                let old: Vec<u64> = old_leaf.iter().map(|t| t.0).collect();
                let new: Vec<u64> = new_leaf.iter().map(|t| t.0).collect();
                let bits: Vec<u64> = leaf_index_bits.iter().map(|b| b.target.0).collect();
                let cap: Vec<u64> = old_cap.0.iter().flat_map(|h| h.elements.iter().map(|t| t.0)).collect();
                let sib: Vec<u64> = proof.siblings.iter().flat_map(|h| h.elements.iter().map(|t| t.0)).collect();
                let h = old_cap.0.len().trailing_zeros() as std::os::raw::c_int;
                let mut out = vec![0u64; cap.len()];
                let rc = unsafe { ffi::p2_builder_merkle_update_to_cap(self.h, old.as_ptr(), new.as_ptr(), old.len(), bits.as_ptr(), bits.len(), cap.as_ptr(), h, sib.as_ptr(), proof.siblings.len(), out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                MerkleCapTarget(out.chunks(4).map(|c| HashOutTarget { elements: core::array::from_fn(|i| Target(c[i])) }).collect())
            }
            pub fn merkle_update<H>(&mut self, old_leaf: Vec<Target>, new_leaf: Vec<Target>, leaf_index_bits: &[BoolTarget], old_root: HashOutTarget, proof: &MerkleProofTarget) -> HashOutTarget {
                self.merkle_update_to_cap::<H>(old_leaf, new_leaf, leaf_index_bits, &MerkleCapTarget(vec![old_root]), proof).0[0]
            }
            /// Not upstream's: sparse keyed trees (`MerkleMap`, include/p2aes.h).  `key_bits` are the little-endian bits of the key.
            /// The map with `cap` holds `value` at the key (`present` = 1) or nothing (`present` = 0, the value then unconstrained).
            pub fn merkle_map_lookup_to_cap<H>(&mut self, key_bits: &[BoolTarget], value: Vec<Target>, present: BoolTarget, cap: &MerkleCapTarget, proof: &MerkleProofTarget) {
                assert!(cap.0.len().is_power_of_two(), "the cap must hold a power of two of hashes");
                let (bits, val, capw, sib) = Self::map_args(key_bits, &value, cap, proof);
                let h = cap.0.len().trailing_zeros() as std::os::raw::c_int;
                let rc = unsafe { ffi::p2_builder_merkle_map_lookup_to_cap(self.h, bits.as_ptr(), bits.len(), val.as_ptr(), val.len(), present.target.0, capw.as_ptr(), h, sib.as_ptr(), proof.siblings.len()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            /// (`old_present`, `old_value`) at the key under `old_cap`; returns the cap with (`new_present`, `new_value`) there.
            pub fn merkle_map_update_to_cap<H>(&mut self, key_bits: &[BoolTarget], old_present: BoolTarget, old_value: Vec<Target>, new_present: BoolTarget, new_value: Vec<Target>, old_cap: &MerkleCapTarget, proof: &MerkleProofTarget) -> MerkleCapTarget {
                assert!(old_cap.0.len().is_power_of_two(), "the cap must hold a power of two of hashes");
                assert!(old_value.len() == new_value.len(), "the old and the new value must have one length");
                let (bits, old, capw, sib) = Self::map_args(key_bits, &old_value, old_cap, proof);
                let new: Vec<u64> = new_value.iter().map(|t| t.0).collect();
                let h = old_cap.0.len().trailing_zeros() as std::os::raw::c_int;
                let mut out = vec![0u64; capw.len()];
                let rc = unsafe { ffi::p2_builder_merkle_map_update_to_cap(self.h, bits.as_ptr(), bits.len(), old_present.target.0, old.as_ptr(), new_present.target.0, new.as_ptr(), old.len(), capw.as_ptr(), h, sib.as_ptr(), proof.siblings.len(), out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                MerkleCapTarget(out.chunks(4).map(|c| HashOutTarget { elements: core::array::from_fn(|i| Target(c[i])) }).collect())
            }
            /// The key is absent under `old_cap`; returns the cap of the map with `value` at it.
            pub fn merkle_map_insert_to_cap<H>(&mut self, key_bits: &[BoolTarget], value: Vec<Target>, old_cap: &MerkleCapTarget, proof: &MerkleProofTarget) -> MerkleCapTarget {
                assert!(old_cap.0.len().is_power_of_two(), "the cap must hold a power of two of hashes");
                let (bits, val, capw, sib) = Self::map_args(key_bits, &value, old_cap, proof);
                let h = old_cap.0.len().trailing_zeros() as std::os::raw::c_int;
                let mut out = vec![0u64; capw.len()];
                let rc = unsafe { ffi::p2_builder_merkle_map_insert_to_cap(self.h, bits.as_ptr(), bits.len(), val.as_ptr(), val.len(), capw.as_ptr(), h, sib.as_ptr(), proof.siblings.len(), out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                MerkleCapTarget(out.chunks(4).map(|c| HashOutTarget { elements: core::array::from_fn(|i| Target(c[i])) }).collect())
            }
            /// The key holds `value` under `old_cap`; returns the cap of the map without it.
            pub fn merkle_map_remove_to_cap<H>(&mut self, key_bits: &[BoolTarget], value: Vec<Target>, old_cap: &MerkleCapTarget, proof: &MerkleProofTarget) -> MerkleCapTarget {
                assert!(old_cap.0.len().is_power_of_two(), "the cap must hold a power of two of hashes");
                let (bits, val, capw, sib) = Self::map_args(key_bits, &value, old_cap, proof);
                let h = old_cap.0.len().trailing_zeros() as std::os::raw::c_int;
                let mut out = vec![0u64; capw.len()];
                let rc = unsafe { ffi::p2_builder_merkle_map_remove_to_cap(self.h, bits.as_ptr(), bits.len(), val.as_ptr(), val.len(), capw.as_ptr(), h, sib.as_ptr(), proof.siblings.len(), out.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                MerkleCapTarget(out.chunks(4).map(|c| HashOutTarget { elements: core::array::from_fn(|i| Target(c[i])) }).collect())
            }
            pub fn merkle_map_lookup<H>(&mut self, key_bits: &[BoolTarget], value: Vec<Target>, present: BoolTarget, root: HashOutTarget, proof: &MerkleProofTarget) {
                self.merkle_map_lookup_to_cap::<H>(key_bits, value, present, &MerkleCapTarget(vec![root]), proof)
            }
            pub fn merkle_map_update<H>(&mut self, key_bits: &[BoolTarget], old_present: BoolTarget, old_value: Vec<Target>, new_present: BoolTarget, new_value: Vec<Target>, old_root: HashOutTarget, proof: &MerkleProofTarget) -> HashOutTarget {
                self.merkle_map_update_to_cap::<H>(key_bits, old_present, old_value, new_present, new_value, &MerkleCapTarget(vec![old_root]), proof).0[0]
            }
            pub fn merkle_map_insert<H>(&mut self, key_bits: &[BoolTarget], value: Vec<Target>, old_root: HashOutTarget, proof: &MerkleProofTarget) -> HashOutTarget {
                self.merkle_map_insert_to_cap::<H>(key_bits, value, &MerkleCapTarget(vec![old_root]), proof).0[0]
            }
            pub fn merkle_map_remove<H>(&mut self, key_bits: &[BoolTarget], value: Vec<Target>, old_root: HashOutTarget, proof: &MerkleProofTarget) -> HashOutTarget {
                self.merkle_map_remove_to_cap::<H>(key_bits, value, &MerkleCapTarget(vec![old_root]), proof).0[0]
            }
            fn map_args(key_bits: &[BoolTarget], value: &[Target], cap: &MerkleCapTarget, proof: &MerkleProofTarget) -> (Vec<u64>, Vec<u64>, Vec<u64>, Vec<u64>) {
                (key_bits.iter().map(|b| b.target.0).collect(), value.iter().map(|t| t.0).collect(),
                 cap.0.iter().flat_map(|h| h.elements.iter().map(|t| t.0)).collect(), proof.siblings.iter().flat_map(|h| h.elements.iter().map(|t| t.0)).collect())
            }
            /// Not upstream's: `multiply_point` (and `public_key`, `elgamal_encrypt`, `hashed_elgamal_encrypt` through it) as 320
            /// EcStepGate rows instead of arithmetic gates.  Off by default.
            pub fn set_ec_gate(&mut self, on: bool) {
                let rc = unsafe { ffi::p2_builder_set_ec_gate(self.h, on as std::os::raw::c_int) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            /// Not upstream's: `AesGcmTarget::build` with a tag computes GHASH from carry-less multiply tables, `lanes` (1 to 16)
            /// blocks per reduction; 0, the default, is the reference's bit-serial circuit.
            pub fn set_ghash_tables(&mut self, lanes: usize) {
                let rc = unsafe { ffi::p2_builder_set_ghash_tables(self.h, lanes as std::os::raw::c_int) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
            }
            pub fn num_gates(&self) -> usize { unsafe { ffi::p2_builder_num_gates(self.h) } }
            /// `build::<PoseidonGoldilocksConfig>()` (19 sites) or `build::<KeccakGoldilocksConfig>()`: compile on the host, then upload the circuit
            /// to HIP device P2AES_DEVICE (default 0) and commit constants | sigmas there.
            pub fn build<C: crate::plonk::config::GenericConfig>(self) -> CircuitData<F, C, D> {
                let rc = unsafe { ffi::p2_builder_set_hasher(self.h, C::HASHER) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                let (mut blob_ptr, mut len) = (core::ptr::null_mut::<u8>(), 0usize);
                let rc = unsafe { ffi::p2_builder_build(self.h, &mut blob_ptr, &mut len) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                let blob = unsafe { std::slice::from_raw_parts(blob_ptr, len) }.to_vec();
                unsafe { ffi::p2_blob_free(blob_ptr) };
                let device = std::env::var("P2AES_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
                let handle = unsafe { ffi::p2_circuit_load(blob.as_ptr(), blob.len(), device) };
                assert!(!handle.is_null(), "{}", last_error());   // no HIP device: the prover has no CPU fallback
                let mut vd = vec![0u64; 80];
                let mut n = 0usize;
                let rc = unsafe { ffi::p2_circuit_verifier_data(handle, vd.as_mut_ptr(), vd.len(), &mut n) };
                assert!(rc == ffi::P2_OK, "{}", last_error());
                vd.truncate(n);
                let num_public_inputs = unsafe { ffi::p2_circuit_num_public_inputs(handle) };
                CircuitData { handle, blob, verifier_data: vd, num_public_inputs, _p: PhantomData }
            }
        }
    }
}

/// The pod2 names the ecgfp5 and poseidon-cipher crates import (`pod2::backends::plonky2::primitives::ec::{curve, bits}`,
/// SURVEY.md A.1 last rows), over `p2_ecgfp5_*` and `p2_builder_*point*`.  Workspace line: `pod2 = { path = ..., package = "plonky2-hip" }`
/// with `pub use plonky2::pod2 as backends` style re-exports in a two-line facade crate.
pub mod pod2 {
    pub mod curve {
        use crate::ffi;
        use crate::iop::target::{BoolTarget, Target};
        use crate::plonk::circuit_builder::CircuitBuilder;
        use crate::field::types::Field;

        /// Affine (x, u) coordinates over GF(p^5), ten words (`Point::as_fields` = x ++ u, hashed_elgamal.rs:23).
        #[derive(Copy, Clone, Debug, Eq, PartialEq)]
        pub struct Point { pub x: [u64; 5], pub u: [u64; 5] }
        fn pack(p: &Point) -> [u64; 10] { let mut o = [0u64; 10]; o[..5].copy_from_slice(&p.x); o[5..].copy_from_slice(&p.u); o }
        fn unpack(o: [u64; 10]) -> Point { let mut p = Point { x: [0; 5], u: [0; 5] }; p.x.copy_from_slice(&o[..5]); p.u.copy_from_slice(&o[5..]); p }
        /// GROUP_ORDER as five little-endian 64-bit limbs (ecgfp5/src/lib.rs:12).
        pub fn group_order() -> [u64; 5] { let mut o = [0u64; 5]; unsafe { ffi::p2_ecgfp5_group_order(o.as_mut_ptr()) }; o }
        impl Point {
            pub fn generator() -> Self { let mut o = [0u64; 10]; unsafe { ffi::p2_ecgfp5_generator(o.as_mut_ptr()) }; unpack(o) }
            pub fn new_rand_from_subgroup() -> Self {
                let mut o = [0u64; 10];
                // OS randomness can fail: an all-zero buffer must never pass for a random point or key
                let rc = unsafe { ffi::p2_ecgfp5_random_point(o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                unpack(o)
            }
            pub fn as_fields(&self) -> Vec<u64> { pack(self).to_vec() }
            pub fn inverse(&self) -> Self { let mut o = [0u64; 10]; unsafe { ffi::p2_ecgfp5_neg(pack(self).as_ptr(), o.as_mut_ptr()) }; unpack(o) }   // elgamal.rs:21
            pub fn is_in_subgroup(&self) -> bool { unsafe { ffi::p2_ecgfp5_is_in_subgroup(pack(self).as_ptr()) == 1 } }
            pub fn compress_from_subgroup(&self) -> [u64; 5] { let mut w = [0u64; 5]; unsafe { ffi::p2_ecgfp5_compress(pack(self).as_ptr(), w.as_mut_ptr()) }; w }   // lib.rs:82
            pub fn decompress_into_subgroup(w: &[u64; 5]) -> anyhow::Result<Self> {                                                                                     // lib.rs:74
                let mut o = [0u64; 10];
                anyhow::ensure!(unsafe { ffi::p2_ecgfp5_decompress(w.as_ptr(), o.as_mut_ptr()) } == ffi::P2_OK, "not the encoding of a group element");
                Ok(unpack(o))
            }
            /// `&k * P` with k as five little-endian limbs (elgamal.rs:13-15).
            pub fn mul_scalar(&self, k: &[u64; 5]) -> Self { let mut o = [0u64; 10]; unsafe { ffi::p2_ecgfp5_mul(k.as_ptr(), pack(self).as_ptr(), o.as_mut_ptr()) }; unpack(o) }
        }
        impl core::ops::Add for Point {
            type Output = Point;
            fn add(self, q: Point) -> Point { let mut o = [0u64; 10]; unsafe { ffi::p2_ecgfp5_add(pack(&self).as_ptr(), pack(&q).as_ptr(), o.as_mut_ptr()) }; unpack(o) }
        }
        #[derive(Copy, Clone, Debug)]
        pub struct PointTarget(pub [Target; 10]);
        #[derive(Clone, Debug)]
        pub struct BigUInt320Target { pub bits: Vec<BoolTarget> }
        fn raw<const N: usize>(ts: &[Target]) -> [u64; N] { core::array::from_fn(|i| ts[i].0) }
        /// `CircuitBuilderElliptic` / `CircuitBuilderBits` (ecgfp5/src/circuit.rs:33-38, elgamal/circuit.rs:34-37,70-72).
        pub trait CircuitBuilderElliptic {
            fn add_virtual_point_target(&mut self) -> PointTarget;
            fn constant_point(&mut self, p: Point) -> PointTarget;
            fn add_virtual_biguint320_target(&mut self) -> BigUInt320Target;
            fn multiply_point(&mut self, bits: &BigUInt320Target, p: &PointTarget) -> PointTarget;
            fn add_point(&mut self, p: &PointTarget, q: &PointTarget) -> PointTarget;
        }
        impl<F: Field, const D: usize> CircuitBuilderElliptic for CircuitBuilder<F, D> {
            fn add_virtual_point_target(&mut self) -> PointTarget {
                let mut o = [0u64; 10];
                unsafe { ffi::p2_builder_add_virtual_point_target(self.h, o.as_mut_ptr()) };
                PointTarget(o.map(Target))
            }
            fn constant_point(&mut self, p: Point) -> PointTarget {
                let mut o = [0u64; 10];
                unsafe { ffi::p2_builder_constant_point(self.h, pack(&p).as_ptr(), o.as_mut_ptr()) };
                PointTarget(o.map(Target))
            }
            fn add_virtual_biguint320_target(&mut self) -> BigUInt320Target {
                let mut o = [0u64; 320];
                unsafe { ffi::p2_builder_add_virtual_biguint320_target(self.h, o.as_mut_ptr()) };
                BigUInt320Target { bits: o.iter().map(|t| BoolTarget::new_unsafe(Target(*t))).collect() }
            }
            fn multiply_point(&mut self, bits: &BigUInt320Target, p: &PointTarget) -> PointTarget {
                let b: Vec<u64> = bits.bits.iter().map(|t| t.target.0).collect();
                let mut o = [0u64; 10];
                let rc = unsafe { ffi::p2_builder_multiply_point(self.h, b.as_ptr(), raw::<10>(&p.0).as_ptr(), o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                PointTarget(o.map(Target))
            }
            fn add_point(&mut self, p: &PointTarget, q: &PointTarget) -> PointTarget {
                let mut o = [0u64; 10];
                unsafe { ffi::p2_builder_add_point(self.h, raw::<10>(&p.0).as_ptr(), raw::<10>(&q.0).as_ptr(), o.as_mut_ptr()) };
                PointTarget(o.map(Target))
            }
        }
        /// Verifiable decryption (not in the reference, whose circuits only encrypt): no new gate.  The caller ties the key to a
        /// public key with `connect(public_key(sk), pk)`.  Not checked in the circuit: `c0` and `c1` in the group, `sk` below the
        /// group order.
        pub trait CircuitBuilderElGamalDecrypt {
            fn neg_point(&mut self, p: &PointTarget) -> PointTarget;
            /// `msg = c1 - sk c0` (elgamal.rs:19).
            fn elgamal_decrypt(&mut self, sk: &BigUInt320Target, c0: &PointTarget, c1: &PointTarget) -> PointTarget;
            /// `msg[i] = ct[i] - hash_n_to_m_no_pad(as_fields(sk c0), 5)[i]` (hashed_elgamal.rs:28).
            fn hashed_elgamal_decrypt(&mut self, sk: &BigUInt320Target, c0: &PointTarget, ct: &[Target; 5]) -> [Target; 5];
        }
        impl<F: Field, const D: usize> CircuitBuilderElGamalDecrypt for CircuitBuilder<F, D> {
            fn neg_point(&mut self, p: &PointTarget) -> PointTarget {
                let mut o = [0u64; 10];
                let rc = unsafe { ffi::p2_builder_neg_point(self.h, raw::<10>(&p.0).as_ptr(), o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                PointTarget(o.map(Target))
            }
            fn elgamal_decrypt(&mut self, sk: &BigUInt320Target, c0: &PointTarget, c1: &PointTarget) -> PointTarget {
                let b: Vec<u64> = sk.bits.iter().map(|t| t.target.0).collect();
                assert!(b.len() == 320, "a secret key holds 320 bits");
                let mut o = [0u64; 10];
                let rc = unsafe { ffi::p2_builder_elgamal_decrypt(self.h, b.as_ptr(), raw::<10>(&c0.0).as_ptr(), raw::<10>(&c1.0).as_ptr(), o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                PointTarget(o.map(Target))
            }
            fn hashed_elgamal_decrypt(&mut self, sk: &BigUInt320Target, c0: &PointTarget, ct: &[Target; 5]) -> [Target; 5] {
                let b: Vec<u64> = sk.bits.iter().map(|t| t.target.0).collect();
                assert!(b.len() == 320, "a secret key holds 320 bits");
                let mut o = [0u64; 5];
                let rc = unsafe { ffi::p2_builder_hashed_elgamal_decrypt(self.h, b.as_ptr(), raw::<10>(&c0.0).as_ptr(), raw::<5>(ct).as_ptr(), o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                o.map(Target)
            }
        }
        /// The Poseidon sponge cipher (poseidon-cipher/src/lib.rs:41, :75) on targets the caller supplies, so that the key can be
        /// `multiply_point(sk, R)`: with `connect(public_key(sk), pk)` that states "this ciphertext decrypts, under the secret key of
        /// this public key, to that message".  An Fq element is five targets; `L` is a multiple of 3; a ciphertext has `L + 1`
        /// elements, the last one the tag.  No new gate.  Not constrained: `ks` on the curve.
        pub trait CircuitBuilderPoseidonCipher {
            /// The loop of `PoseidonEncryptTarget::build` (circuit.rs:66-86).
            fn poseidon_encrypt(&mut self, ks: &PointTarget, nonce: &[Target; 2], m: &[[Target; 5]]) -> Vec<[Target; 5]>;
            /// `m = ct - s[1..3]` per block; the tag is connected to the closing state, so a wrong one is an unsatisfiable witness.
            fn poseidon_decrypt(&mut self, ks: &PointTarget, nonce: &[Target; 2], ct: &[[Target; 5]]) -> Vec<[Target; 5]>;
        }
        impl<F: Field, const D: usize> CircuitBuilderPoseidonCipher for CircuitBuilder<F, D> {
            fn poseidon_encrypt(&mut self, ks: &PointTarget, nonce: &[Target; 2], m: &[[Target; 5]]) -> Vec<[Target; 5]> {
                assert!(m.len() % 3 == 0, "L must be a multiple of 3");
                let i: Vec<u64> = m.iter().flat_map(|e| e.iter().map(|t| t.0)).collect();
                let mut o = vec![0u64; 5 * (m.len() + 1)];
                let rc = unsafe { ffi::p2_builder_poseidon_encrypt(self.h, raw::<10>(&ks.0).as_ptr(), raw::<2>(nonce).as_ptr(), i.as_ptr(), m.len(), o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                o.chunks(5).map(|c| core::array::from_fn(|j| Target(c[j]))).collect()
            }
            fn poseidon_decrypt(&mut self, ks: &PointTarget, nonce: &[Target; 2], ct: &[[Target; 5]]) -> Vec<[Target; 5]> {
                assert!(ct.len() % 3 == 1, "a ciphertext has L + 1 elements, L a multiple of 3");
                let i: Vec<u64> = ct.iter().flat_map(|e| e.iter().map(|t| t.0)).collect();
                let mut o = vec![0u64; 5 * (ct.len() - 1)];
                let rc = unsafe { ffi::p2_builder_poseidon_decrypt(self.h, raw::<10>(&ks.0).as_ptr(), raw::<2>(nonce).as_ptr(), i.as_ptr(), ct.len() - 1, o.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                o.chunks(5).map(|c| core::array::from_fn(|j| Target(c[j]))).collect()
            }
        }
    }
    /// Schnorr signatures on ecGFp5 with a Poseidon challenge (csrc/schnorr.h; this project's own scheme, UNPINNED against pod2's
    /// signature bytes): `p2_schnorr_*` on the host and the `verify_schnorr_signature` gadget.
    pub mod schnorr {
        use super::curve::{BigUInt320Target, Point, PointTarget};
        use crate::ffi;
        use crate::field::types::Field;
        use crate::hash::hash_types::HashOutTarget;
        use crate::iop::target::{BoolTarget, Target};
        use crate::plonk::circuit_builder::CircuitBuilder;

        /// s as five little-endian limbs, then the four challenge words.
        #[derive(Copy, Clone, Debug, Eq, PartialEq)]
        pub struct Signature { pub s: [u64; 5], pub e: [u64; 4] }
        #[derive(Copy, Clone, Debug, Eq, PartialEq)]
        pub enum Verdict { Accepted, Rejected, Malformed }
        fn pack(p: &Point) -> [u64; 10] { let mut o = [0u64; 10]; o[..5].copy_from_slice(&p.x); o[5..].copy_from_slice(&p.u); o }
        /// (a b + c) mod the group order for arbitrary 320-bit operands.
        pub fn scalar_muladd(a: &[u64; 5], b: &[u64; 5], c: &[u64; 5]) -> [u64; 5] {
            let mut o = [0u64; 5];
            unsafe { ffi::p2_ecgfp5_scalar_muladd(a.as_ptr(), b.as_ptr(), c.as_ptr(), o.as_mut_ptr()) };
            o
        }
        /// Sign with a caller-supplied nonce in [1, n); `Err` for a key or nonce outside [1, n) or a message word not below p.
        pub fn sign(sk: &[u64; 5], msg: &[u64], nonce: &[u64; 5]) -> Result<Signature, String> {
            let mut sig = [0u64; 9];
            let mut status: std::os::raw::c_int = -1;
            let rc = unsafe { ffi::p2_schnorr_sign(sk.as_ptr(), nonce.as_ptr(), msg.as_ptr(), msg.len(), sig.as_mut_ptr(), core::ptr::null_mut(), &mut status) };
            if rc != ffi::P2_OK { return Err(crate::last_error()); }
            if status != 0 { return Err("secret key and nonce must be in [1, n), message words below p".into()); }
            Ok(Signature { s: core::array::from_fn(|i| sig[i]), e: core::array::from_fn(|i| sig[5 + i]) })
        }
        pub fn verify(pk: &Point, msg: &[u64], sig: &Signature) -> Result<Verdict, String> {
            let mut w = [0u64; 9];
            w[..5].copy_from_slice(&sig.s);
            w[5..].copy_from_slice(&sig.e);
            let mut status: std::os::raw::c_int = -1;
            let rc = unsafe { ffi::p2_schnorr_verify(pack(pk).as_ptr(), msg.as_ptr(), msg.len(), w.as_ptr(), &mut status) };
            if rc != ffi::P2_OK { return Err(crate::last_error()); }
            Ok(match status { 0 => Verdict::Accepted, 1 => Verdict::Rejected, _ => Verdict::Malformed })
        }
        #[derive(Clone, Debug)]
        pub struct SignatureTarget { pub s: BigUInt320Target, pub e: HashOutTarget }
        pub trait CircuitBuilderSchnorr {
            fn add_virtual_schnorr_signature_target(&mut self) -> SignatureTarget;
            /// Constrains hash(R' | pk | msg) = e for R' = s G + e (-pk) and returns R'.  Not checked in the circuit: s below the
            /// group order, pk in the group.
            fn verify_schnorr_signature(&mut self, pk: &PointTarget, msg: &[Target], sig: &SignatureTarget) -> PointTarget;
        }
        impl<F: Field, const D: usize> CircuitBuilderSchnorr for CircuitBuilder<F, D> {
            fn add_virtual_schnorr_signature_target(&mut self) -> SignatureTarget {
                let mut bits = [0u64; 320];
                let mut e = [0u64; 4];
                let rc = unsafe { ffi::p2_builder_add_virtual_schnorr_signature(self.h, bits.as_mut_ptr(), e.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                SignatureTarget { s: BigUInt320Target { bits: bits.iter().map(|t| BoolTarget::new_unsafe(Target(*t))).collect() }, e: HashOutTarget { elements: e.map(Target) } }
            }
            fn verify_schnorr_signature(&mut self, pk: &PointTarget, msg: &[Target], sig: &SignatureTarget) -> PointTarget {
                let p: [u64; 10] = core::array::from_fn(|i| pk.0[i].0);
                let m: Vec<u64> = msg.iter().map(|t| t.0).collect();
                let b: Vec<u64> = sig.s.bits.iter().map(|t| t.target.0).collect();
                assert!(b.len() == 320, "a signature holds 320 bits of s");
                let e: [u64; 4] = core::array::from_fn(|i| sig.e.elements[i].0);
                let mut r = [0u64; 10];
                let rc = unsafe { ffi::p2_builder_verify_schnorr_signature(self.h, p.as_ptr(), m.as_ptr(), m.len(), b.as_ptr(), e.as_ptr(), r.as_mut_ptr()) };
                assert!(rc == ffi::P2_OK, "{}", crate::last_error());
                PointTarget(r.map(Target))
            }
        }
    }
}

#[allow(unused)]
fn _phantom_use(_: PhantomData<()>) {}
