//! MI355X backend of the profile-HMM read-likelihood path: the `impl PHMMModel` methods of
//! `hmmv2/freq.rs` and `hmmv2/hint.rs` re-implemented over `libphmm_amd.so` (amd_sys.rs).
//!
//! Place as `src/hmmv2/amd.rs`, add `pub mod amd; pub mod amd_sys;` to `src/hmmv2.rs` behind a cargo
//! feature (`amd`), and gate the CPU bodies of the same-named methods with `#[cfg(not(feature = "amd"))]`:
//! `MultiDbg::to_likelihood` (multi_dbg/posterior.rs:247-255) and `MultiDbg::generate_mappings`
//! (multi_dbg/posterior.rs:609-630) then call into the GPU unchanged.  Error behaviour is the
//! reference's: it has no `Result` on this path, a failing call panics with the library's message.
//!
//! Handles: `AmdModel` (topology + probabilities of one PHMM), `AmdReads`, `AmdMappings` own their
//! device arrays and free them on drop.  The DP workspaces belong to the device and are shared by all
//! handles (`phmm_release_workspace`), so a mapping model and a scoring model can be alive together.
use super::amd_sys::*;
use super::common::{PHMMEdge, PHMMModel, PHMMNode};
use super::hint::{Mapping, Mappings};
use super::params::PHMMParams;
use super::sample::State;
use crate::common::collection::ReadCollection;
use crate::common::{CopyNum, Seq};
use crate::multi_dbg::neighbors::UpdateInfo;
use crate::multi_dbg::{CopyNums, MultiDbg};
use crate::prob::Prob;
use petgraph::graph::{EdgeIndex, NodeIndex};
use std::ffi::CStr;
use std::os::raw::c_int;
use std::ptr;

/// non-zero status -> panic!, preserving the reference's error behaviour
fn check(rc: c_int) {
    if rc != PHMM_OK {
        let msg = unsafe { CStr::from_ptr(phmm_last_error()) }.to_string_lossy().into_owned();
        panic!("phmm_amd error {}: {}", rc, msg);
    }
}

fn to_params_c(p: &PHMMParams) -> phmm_params {
    phmm_params {
        p_mismatch: p.p_mismatch.to_log_value(),
        p_match: p.p_match.to_log_value(),
        p_random: p.p_random.to_log_value(),
        p_gap_open: p.p_gap_open.to_log_value(),
        p_gap_ext: p.p_gap_ext.to_log_value(),
        p_end: p.p_end.to_log_value(),
        p_mm: p.p_MM.to_log_value(),
        p_im: p.p_IM.to_log_value(),
        p_dm: p.p_DM.to_log_value(),
        p_mi: p.p_MI.to_log_value(),
        p_ii: p.p_II.to_log_value(),
        p_di: p.p_DI.to_log_value(),
        p_md: p.p_MD.to_log_value(),
        p_id: p.p_ID.to_log_value(),
        p_dd: p.p_DD.to_log_value(),
        n_active_nodes: p.n_active_nodes as i64,
        active_node_max_ratio: p.active_node_max_ratio,
        n_warmup: p.n_warmup as i64,
        warmup_threshold: p.warmup_threshold as i64,
        n_max_gaps: p.n_max_gaps as i64,
    }
}

pub struct AmdModel(*mut phmm_model);
impl Drop for AmdModel {
    fn drop(&mut self) {
        unsafe { phmm_model_destroy(self.0) }
    }
}
impl AmdModel {
    /// Flatten the petgraph into the arrays the ABI takes: node id = NodeIndex, edge order = EdgeIndex
    /// order = petgraph insertion order (the library rebuilds petgraph's newest-edge-first adjacency
    /// order from it), Prob -> to_log_value().
    pub fn new<N: PHMMNode, E: PHMMEdge>(phmm: &PHMMModel<N, E>) -> AmdModel {
        let emission: Vec<u8> = phmm.nodes().map(|(_, w)| w.emission()).collect();
        let init: Vec<f64> = phmm.nodes().map(|(_, w)| w.init_prob().to_log_value()).collect();
        let (mut src, mut dst, mut tr) = (Vec::new(), Vec::new(), Vec::new());
        for (_, s, t, w) in phmm.edges() {
            src.push(s.index() as u32);
            dst.push(t.index() as u32);
            tr.push(w.trans_prob().to_log_value());
        }
        let p = to_params_c(&phmm.param);
        let mut h = ptr::null_mut();
        check(unsafe {
            phmm_model_create(emission.len() as u32, src.len() as u32, emission.as_ptr(), init.as_ptr(), src.as_ptr(),
                              dst.as_ptr(), tr.as_ptr(), &p, &mut h)
        });
        AmdModel(h)
    }
    /// next candidate on the same topology (what `dbg.clone(); set_copy_nums; to_phmm` rebuilds, posterior.rs:483-501)
    pub fn set_probs<N: PHMMNode, E: PHMMEdge>(&mut self, phmm: &PHMMModel<N, E>) {
        let init: Vec<f64> = phmm.nodes().map(|(_, w)| w.init_prob().to_log_value()).collect();
        let tr: Vec<f64> = phmm.edges().map(|(_, _, _, w)| w.trans_prob().to_log_value()).collect();
        check(unsafe { phmm_model_set_probs(self.0, init.as_ptr(), tr.as_ptr()) });
    }
}

pub struct AmdReads {
    h: *mut phmm_reads,
    offsets: Vec<u64>,
}
impl Drop for AmdReads {
    fn drop(&mut self) {
        unsafe { phmm_reads_destroy(self.h) }
    }
}
impl AmdReads {
    /// concatenated bases + offsets (ReadCollection<S>, common/collection.rs:38-83)
    pub fn new<S: Seq>(reads: &ReadCollection<S>) -> AmdReads {
        let mut bases: Vec<u8> = Vec::new();
        let mut offsets: Vec<u64> = vec![0];
        for r in reads.iter() {
            bases.extend_from_slice(r.as_ref());
            offsets.push(bases.len() as u64);
        }
        let mut h = ptr::null_mut();
        check(unsafe { phmm_reads_create(bases.as_ptr(), offsets.as_ptr(), (offsets.len() - 1) as u64, &mut h) });
        AmdReads { h, offsets }
    }
    pub fn n_reads(&self) -> usize {
        self.offsets.len() - 1
    }
}

pub struct AmdMappings(*mut phmm_mappings);
impl Drop for AmdMappings {
    fn drop(&mut self) {
        unsafe { phmm_mappings_destroy(self.0) }
    }
}
impl AmdMappings {
    /// Mappings (hint.rs:27-30, 149) -> the 3-level CSR of the ABI
    pub fn from_mappings(reads: &AmdReads, mappings: &Mappings) -> AmdMappings {
        let (mut pos_off, mut nodes, mut logp) = (vec![0u64], Vec::<u32>::new(), Vec::<f64>::new());
        for i in 0..mappings.n_reads() {
            let m: &Mapping = &mappings[i];
            for j in 0..m.len() {
                for (&v, &p) in m.nodes[j].iter().zip(m.probs[j].iter()) {  // (pub fields, hint.rs:27-30)
                    nodes.push(v.index() as u32);
                    logp.push(p.to_log_value());
                }
                pos_off.push(nodes.len() as u64);
            }
        }
        let mut h = ptr::null_mut();
        check(unsafe { phmm_mappings_create(reads.h, pos_off.as_ptr(), nodes.as_ptr(), logp.as_ptr(), &mut h) });
        AmdMappings(h)
    }
    /// the ABI's CSR -> Mappings (phmm_mappings_export), one Mapping per read
    pub fn into_mappings(self, reads: &AmdReads) -> Mappings {
        let (tp, te) = unsafe { (phmm_mappings_total_positions(self.0), phmm_mappings_total_entries(self.0)) };
        let mut pos_off = vec![0u64; tp as usize + 1];
        let mut nodes = vec![0u32; te as usize];
        let mut logp = vec![0f64; te as usize];
        check(unsafe { phmm_mappings_export(self.0, pos_off.as_mut_ptr(), nodes.as_mut_ptr(), logp.as_mut_ptr()) });
        let mut out = Vec::with_capacity(reads.n_reads());
        for r in 0..reads.n_reads() {
            let vs: Vec<Vec<(NodeIndex, Prob)>> = (reads.offsets[r]..reads.offsets[r + 1])
                .map(|g| {
                    (pos_off[g as usize]..pos_off[g as usize + 1])
                        .map(|a| (NodeIndex::new(nodes[a as usize] as usize), Prob::from_log_prob(logp[a as usize])))
                        .collect()
                })
                .collect();
            out.push(Mapping::from_nodes_and_probs(&vs));
        }
        Mappings::new(out)
    }
    /// ln P of every read by the forward pass that produced these mappings (PHMMOutput::to_full_prob_forward,
    /// table.rs:482-491) -> (total, per read).  Mappings from `generate_mappings` only.
    pub fn read_logp(&self, reads: &AmdReads) -> (f64, Vec<f64>) {
        let (mut total, mut per) = (0f64, vec![0f64; reads.n_reads()]);
        check(unsafe { phmm_mappings_read_logp(self.0, per.as_mut_ptr(), &mut total) });
        (total, per)
    }
    /// the same by the backward pass of that call, B.tables[0].mb (PHMMOutput::to_full_prob_backward, table.rs:492-494;
    /// backward_by_forward or backward_with_mapping, backward.rs:59-142) -> (total, per read).  Mappings from
    /// `generate_mappings` only.
    pub fn read_logp_backward(&self, reads: &AmdReads) -> (f64, Vec<f64>) {
        let (mut total, mut per) = (0f64, vec![0f64; reads.n_reads()]);
        check(unsafe { phmm_mappings_read_logp_backward(self.0, per.as_mut_ptr(), &mut total) });
        (total, per)
    }
}

impl<N: PHMMNode, E: PHMMEdge> PHMMModel<N, E> {
    /// drop-in for `to_full_prob_reads` (freq.rs:175-192): forward_with_mapping_score_only per read when
    /// mappings are given, else forward_sparse_score_only(use_max_ratio); the product over reads.
    pub fn to_full_prob_reads_amd<S: Seq>(&self, reads: &ReadCollection<S>, mappings: Option<&Mappings>,
                                          use_max_ratio: bool) -> Prob {
        let m = AmdModel::new(self);
        let r = AmdReads::new(reads);
        let mp = mappings.map(|mp| AmdMappings::from_mappings(&r, mp));
        let mut total = 0f64;
        check(unsafe {
            phmm_full_prob_reads(m.0, r.h, mp.as_ref().map_or(ptr::null(), |x| x.0 as *const _), use_max_ratio as c_int,
                                 ptr::null_mut(), &mut total)
        });
        Prob::from_log_prob(total)
    }

    /// drop-in for `generate_mappings` (hint.rs:193-220): run_with_mapping when `mappings` is given (hint.rs:206-208),
    /// else run_sparse_adaptive(use_max_ratio); then to_mapping_by_score_ratio / to_mapping.
    pub fn generate_mappings_amd<S: Seq>(&self, reads: &ReadCollection<S>, mappings: Option<&Mappings>,
                                         use_max_ratio: bool) -> Mappings {
        let m = AmdModel::new(self);
        let r = AmdReads::new(reads);
        let mp = mappings.map(|mp| AmdMappings::from_mappings(&r, mp));
        let mut out = ptr::null_mut();
        check(unsafe {
            phmm_generate_mappings(m.0, r.h, mp.as_ref().map_or(ptr::null(), |x| x.0 as *const _), use_max_ratio as c_int,
                                   &mut out, ptr::null_mut())
        });
        AmdMappings(out).into_mappings(&r)
    }

    /// `generate_mappings` on a read handle the caller keeps (`AmdReads::new(reads)` once per read set).  `infer` passes the
    /// SAME reads at every k (multi_dbg/posterior.rs:698-826): the handle remembers how many dense warm-up columns
    /// each read needed in its last adaptive call, the next call groups reads by that (results do not depend on the
    /// grouping), and only the very first call of a read set runs without hints (bench.py: cold_hint_ms vs ms_per_step).
    pub fn generate_mappings_amd_on(&self, reads: &AmdReads, mappings: Option<&Mappings>, use_max_ratio: bool) -> Mappings {
        let m = AmdModel::new(self);
        let mp = mappings.map(|mp| AmdMappings::from_mappings(reads, mp));
        let mut out = ptr::null_mut();
        check(unsafe {
            phmm_generate_mappings(m.0, reads.h, mp.as_ref().map_or(ptr::null(), |x| x.0 as *const _), use_max_ratio as c_int,
                                   &mut out, ptr::null_mut())
        });
        AmdMappings(out).into_mappings(reads)
    }

    /// `generate_mappings_amd_on` plus the forward and the backward ln P of every read from the same pass -- what
    /// bin/mapping.rs:94-113 prints as pF / pB.  Their gap is the reference's check of a read (hmmv2/tests/dbg.rs:170-172):
    /// the probability mass the truncated frontier lost.  -> (mappings, ln P forward, ln P backward)
    pub fn generate_mappings_amd_with_probs(&self, reads: &AmdReads, mappings: Option<&Mappings>, use_max_ratio: bool)
                                            -> (Mappings, Vec<f64>, Vec<f64>) {
        let m = AmdModel::new(self);
        let mp = mappings.map(|mp| AmdMappings::from_mappings(reads, mp));
        let mut out = ptr::null_mut();
        check(unsafe {
            phmm_generate_mappings(m.0, reads.h, mp.as_ref().map_or(ptr::null(), |x| x.0 as *const _), use_max_ratio as c_int,
                                   &mut out, ptr::null_mut())
        });
        let h = AmdMappings(out);
        let (_, pf) = h.read_logp(reads);
        let (_, pb) = h.read_logp_backward(reads);
        (h.into_mappings(reads), pf, pb)
    }

    /// drop-in for `to_full_prob_sparse_backward` (freq.rs:153-163; backward_sparse per read, backward.rs:146-185)
    pub fn to_full_prob_sparse_backward_amd<S: Seq>(&self, reads: &ReadCollection<S>) -> Prob {
        let (m, r) = (AmdModel::new(self), AmdReads::new(reads));
        let mut total = 0f64;
        check(unsafe { phmm_full_prob_sparse_backward(m.0, r.h, ptr::null_mut(), &mut total) });
        Prob::from_log_prob(total)
    }

    /// `run` over a read set + to_full_prob_forward + to_node_freqs summed (freq.rs:89-119, 245-255) -> (ln P per read, node usage)
    pub fn run_dense_amd<S: Seq>(&self, reads: &ReadCollection<S>) -> (Vec<Prob>, Vec<f64>) {
        let (m, r) = (AmdModel::new(self), AmdReads::new(reads));
        let mut lf = vec![0f64; r.n_reads()];
        let mut nf = vec![0f64; self.n_nodes()];
        check(unsafe { phmm_run_dense(m.0, r.h, lf.as_mut_ptr(), ptr::null_mut(), nf.as_mut_ptr()) });
        (lf.into_iter().map(Prob::from_log_prob).collect(), nf)
    }

    /// run_sparse (freq.rs:51-55) over a read set + to_node_freqs (freq.rs:245-255), summed over the reads (dense Vec:
    /// the reference's NodeFreqs is a SparseVec alias, freq.rs:200)
    pub fn to_node_freqs_sparse_amd<S: Seq>(&self, reads: &ReadCollection<S>) -> Vec<f64> {
        let (m, r) = (AmdModel::new(self), AmdReads::new(reads));
        let mut nf = vec![0f64; self.n_nodes()];
        check(unsafe { phmm_run_sparse(m.0, r.h, ptr::null_mut(), ptr::null_mut(), nf.as_mut_ptr()) });
        nf
    }

    /// to_edge_and_init_freqs summed over the reads (freq.rs:276-298) and q_score_exact (q.rs:66-96) -> (init, trans, prior)
    pub fn q_score_amd<S: Seq>(&self, reads: &ReadCollection<S>) -> (f64, f64, f64) {
        let (m, r) = (AmdModel::new(self), AmdReads::new(reads));
        let (mut ef, mut nf, mut q) = (vec![0f64; self.n_edges().max(1)], vec![0f64; self.n_nodes()], [0f64; 3]);
        check(unsafe { phmm_run_dense_edges(m.0, r.h, ptr::null_mut(), ef.as_mut_ptr(), nf.as_mut_ptr()) });
        check(unsafe { phmm_q_score_exact(m.0, ef.as_ptr(), nf.as_ptr(), q.as_mut_ptr()) });
        (q[0], q[1], q[2])
    }

    /// run_with_mapping (freq.rs:72-76) of every read on its lists + to_edge_and_init_freqs (freq.rs:276-298), summed
    /// over the reads -> (edge freqs, init freqs).  The cost of a hinted generate_mappings, no dense table.
    pub fn to_edge_and_init_freqs_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings) -> (Vec<f64>, Vec<f64>) {
        let m = AmdModel::new(self);
        let mp = AmdMappings::from_mappings(reads, mappings);
        let (mut ef, mut nf) = (vec![0f64; self.n_edges().max(1)], vec![0f64; self.n_nodes()]);
        check(unsafe {
            phmm_run_with_mapping_edges(m.0, reads.h, mp.0, ptr::null_mut(), ef.as_mut_ptr(), nf.as_mut_ptr())
        });
        ef.truncate(self.n_edges());
        (ef, nf)
    }

    /// run_with_mapping (freq.rs:72-76) of every read on its lists, then per read and read position p
    /// `to_emit_probs(p + 1).to_states()` (table.rs:500-505, 215-254): the Match / Ins / Del states of the listed nodes
    /// with their posteriors, most probable first (equal values in the reference's order: Del before Ins before Match,
    /// the later list entry first).  Built on the host from the three planes of phmm_run_with_mapping_states.
    /// Unverified, like the rest of this shim: it has not been compiled here.
    pub fn to_states_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings) -> Vec<Vec<Vec<(State, Prob)>>> {
        let m = AmdModel::new(self);
        let mp = AmdMappings::from_mappings(reads, mappings);
        let te = unsafe { phmm_mappings_total_entries(mp.0) } as usize;
        let mut sl = vec![0f64; 3 * te.max(1)];
        check(unsafe {
            phmm_run_with_mapping_states(m.0, reads.h, mp.0, ptr::null_mut(), sl.as_mut_ptr(), ptr::null_mut())
        });
        let mut a = 0usize;  // entry of the CSR: the order from_mappings wrote
        let mut out = Vec::with_capacity(mappings.n_reads());
        for i in 0..mappings.n_reads() {
            let mapping: &Mapping = &mappings[i];
            let mut per_pos = Vec::with_capacity(mapping.len());
            for j in 0..mapping.len() {
                let nodes = &mapping.nodes[j];
                let mut states: Vec<(State, Prob)> = Vec::with_capacity(3 * nodes.len());
                for kind in 0..3 {
                    for (slot, &v) in nodes.iter().enumerate() {
                        let p = Prob::from_log_prob(sl[3 * (a + slot) + kind]);
                        states.push(match kind {
                            0 => (State::Match(v), p),
                            1 => (State::Ins(v), p),
                            _ => (State::Del(v), p),
                        });
                    }
                }
                states.sort_by_key(|(_, p)| *p);  // (stable, then reversed: table.rs:237-238)
                states.reverse();
                a += nodes.len();
                per_pos.push(states);
            }
            out.push(per_pos);
        }
        out
    }

    /// The best path (Viterbi) of every read over its lists: forward_with_mapping (forward.rs:51-75) with every sum
    /// replaced by a maximum, and the walk back (phmm_run_with_mapping_best_path, include/phmm_amd_path.h).  Per read
    /// the probability of the path and the states it passes in order, Del states included; (Prob::zero(), empty) for a
    /// read without a path of positive probability on its lists.  The reference has no such call.
    /// Unverified, like the rest of this shim: it has not been compiled here.
    pub fn best_path_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings) -> Vec<(Prob, Vec<State>)> {
        let m = AmdModel::new(self);
        let mp = AmdMappings::from_mappings(reads, mappings);
        let stride = self.param.n_max_gaps + 2;
        let n_bases: usize = (0..mappings.n_reads()).map(|i| mappings[i].len()).sum();
        let mut logp = vec![0f64; mappings.n_reads().max(1)];
        let mut path = vec![PHMM_PATH_NONE; (stride * n_bases).max(1)];
        check(unsafe {
            phmm_run_with_mapping_best_path(m.0, reads.h, mp.0, logp.as_mut_ptr(), path.as_mut_ptr(), ptr::null_mut())
        });
        let mut g = 0usize;  // global base: the order from_mappings wrote
        let mut out = Vec::with_capacity(mappings.n_reads());
        for i in 0..mappings.n_reads() {
            let mapping: &Mapping = &mappings[i];
            let mut states = Vec::new();
            for j in 0..mapping.len() {
                for &code in &path[stride * g..stride * (g + 1)] {
                    if code == PHMM_PATH_NONE {
                        break;
                    }
                    states.push(if code == PHMM_PATH_INS_BEGIN {
                        State::InsBegin
                    } else {
                        let v = mapping.nodes[j][(code >> 2) as usize];
                        match code & 3 {
                            0 => State::Match(v),
                            1 => State::Ins(v),
                            _ => State::Del(v),
                        }
                    });
                }
                g += 1;
            }
            out.push((Prob::from_log_prob(logp[i]), states));
        }
        out
    }

    /// The maximum-expected-accuracy path of every read over its lists (phmm_run_with_mapping_mea_path,
    /// include/phmm_amd_mea.h): the legal walk whose states have the largest summed posterior, Del states weighted by
    /// del_weight (1: emitting and Del states count alike, 0: emitting states only).  Per read the score -- the expected
    /// number of the path's states that the true path shares at the same base -- and the states in order, Del states
    /// included, decoded as best_path_with_mapping_amd decodes them.  The reference has no such call.
    /// Unverified, like the rest of this shim: it has not been compiled here.
    pub fn mea_path_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings, del_weight: f64) -> Vec<(f64, Vec<State>)> {
        let m = AmdModel::new(self);
        let mp = AmdMappings::from_mappings(reads, mappings);
        let stride = self.param.n_max_gaps + 2;
        let n_bases: usize = (0..mappings.n_reads()).map(|i| mappings[i].len()).sum();
        let mut score = vec![0f64; mappings.n_reads().max(1)];
        let mut path = vec![PHMM_PATH_NONE; (stride * n_bases).max(1)];
        check(unsafe {
            phmm_run_with_mapping_mea_path(m.0, reads.h, mp.0, del_weight, ptr::null_mut(), score.as_mut_ptr(),
                                           path.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())
        });
        let mut g = 0usize;  // global base: the order from_mappings wrote
        let mut out = Vec::with_capacity(mappings.n_reads());
        for i in 0..mappings.n_reads() {
            let mapping: &Mapping = &mappings[i];
            let mut states = Vec::new();
            for j in 0..mapping.len() {
                for &code in &path[stride * g..stride * (g + 1)] {
                    if code == PHMM_PATH_NONE {
                        break;
                    }
                    states.push(if code == PHMM_PATH_INS_BEGIN {
                        State::InsBegin
                    } else {
                        let v = mapping.nodes[j][(code >> 2) as usize];
                        match code & 3 {
                            0 => State::Match(v),
                            1 => State::Ins(v),
                            _ => State::Del(v),
                        }
                    });
                }
                g += 1;
            }
            out.push((score[i], states));
        }
        out
    }

    /// forward_with_mapping (forward.rs:51-75) and backward_with_mapping (backward.rs:59-93) of every read on its lists
    /// with the tables themselves returned (phmm_run_with_mapping_tables, include/phmm_amd_tables.h): per read the pair
    /// (forward, backward) of PHMMTables that run_with_mapping builds, each table sparse over the nodes of its list, with
    /// ib / e (forward) and mb / ib (backward) set and the init tables built from the parameters as f_init / b_init do.
    /// A read of probability 0 on its lists is a result: its tables hold Prob::zero() from where the mass ends.
    /// Unverified, like the rest of this shim: it has not been compiled here.
    pub fn tables_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings) -> Vec<(PHMMTables, PHMMTables)> {
        let m = AmdModel::new(self);
        let mp = AmdMappings::from_mappings(reads, mappings);
        let n_bases: usize = (0..mappings.n_reads()).map(|i| mappings[i].len()).sum();
        let n_entries: usize = (0..mappings.n_reads())
            .map(|i| (0..mappings[i].len()).map(|j| mappings[i].nodes[j].len()).sum::<usize>())
            .sum();
        let mut f = vec![0f64; (3 * n_entries).max(1)];
        let mut b = vec![0f64; (3 * n_entries).max(1)];
        let mut fs = vec![0f64; (2 * n_bases).max(1)];
        let mut bs = vec![0f64; (2 * n_bases).max(1)];
        check(unsafe {
            phmm_run_with_mapping_tables(m.0, reads.h, mp.0, ptr::null_mut(), ptr::null_mut(), f.as_mut_ptr(),
                                         fs.as_mut_ptr(), b.as_mut_ptr(), bs.as_mut_ptr())
        });
        let (mut g, mut a) = (0usize, 0usize);  // global base and entry: the order from_mappings wrote
        let mut out = Vec::with_capacity(mappings.n_reads());
        for i in 0..mappings.n_reads() {
            let mapping: &Mapping = &mappings[i];
            let mut ft = PHMMTables { init_table: self.f_init(false), tables: Vec::new(), kind: PHMMKind::Forward };
            let mut bt = PHMMTables { init_table: self.b_init(false), tables: Vec::new(), kind: PHMMKind::Backward };
            for j in 0..mapping.len() {
                let mut tf = PHMMTable::zero(false, self.n_nodes());
                let mut tb = PHMMTable::zero(false, self.n_nodes());
                for &v in mapping.nodes[j].iter() {
                    tf.m[v] = Prob::from_log_prob(f[3 * a]);
                    tf.i[v] = Prob::from_log_prob(f[3 * a + 1]);
                    tf.d[v] = Prob::from_log_prob(f[3 * a + 2]);
                    tb.m[v] = Prob::from_log_prob(b[3 * a]);
                    tb.i[v] = Prob::from_log_prob(b[3 * a + 1]);
                    tb.d[v] = Prob::from_log_prob(b[3 * a + 2]);
                    a += 1;
                }
                tf.ib = Prob::from_log_prob(fs[2 * g]);
                tf.e = Prob::from_log_prob(fs[2 * g + 1]);
                tb.mb = Prob::from_log_prob(bs[2 * g]);
                tb.ib = Prob::from_log_prob(bs[2 * g + 1]);
                ft.tables.push(tf);
                bt.tables.push(tb);
                g += 1;
            }
            out.push((ft, bt));
        }
        out
    }

    /// n_samples (1..=64) draws from the posterior over paths of every read over its lists
    /// (phmm_run_with_mapping_sample_paths, include/phmm_amd_sample.h): the forward sums as the filter and one random
    /// walk back per sample.  Per read the forward total over its lists and, per sample, the probability of the sampled
    /// path and the states it passes in order, Del states included; (Prob::zero(), empty) for a read without a path.
    /// A read's samples depend on seed, its index and the sample number alone.  The reference has no such call.
    /// Unverified, like the rest of this shim: it has not been compiled here.
    pub fn sample_paths_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings, n_samples: usize, seed: u64)
                                         -> Vec<(Prob, Vec<(Prob, Vec<State>)>)> {
        let m = AmdModel::new(self);
        let mp = AmdMappings::from_mappings(reads, mappings);
        let stride = self.param.n_max_gaps + 2;
        let n_reads = mappings.n_reads();
        let n_bases: usize = (0..n_reads).map(|i| mappings[i].len()).sum();
        let mut logp = vec![0f64; n_reads.max(1)];
        let mut path_logp = vec![0f64; (n_reads * n_samples).max(1)];
        let mut path = vec![PHMM_PATH_NONE; (n_samples * stride * n_bases).max(1)];
        check(unsafe {
            phmm_run_with_mapping_sample_paths(m.0, reads.h, mp.0, n_samples as u32, seed, logp.as_mut_ptr(),
                                               path_logp.as_mut_ptr(), path.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())
        });
        let mut g0 = 0usize;  // first global base of the read: the order from_mappings wrote
        let mut out = Vec::with_capacity(n_reads);
        for i in 0..n_reads {
            let mapping: &Mapping = &mappings[i];
            let mut samples = Vec::with_capacity(n_samples);
            for s in 0..n_samples {
                let plane = &path[s * stride * n_bases..(s + 1) * stride * n_bases];
                let mut states = Vec::new();
                for j in 0..mapping.len() {
                    for &code in &plane[stride * (g0 + j)..stride * (g0 + j + 1)] {
                        if code == PHMM_PATH_NONE {
                            break;
                        }
                        states.push(if code == PHMM_PATH_INS_BEGIN {
                            State::InsBegin
                        } else {
                            let v = mapping.nodes[j][(code >> 2) as usize];
                            match code & 3 {
                                0 => State::Match(v),
                                1 => State::Ins(v),
                                _ => State::Del(v),
                            }
                        });
                    }
                }
                samples.push((Prob::from_log_prob(path_logp[i * n_samples + s]), states));
            }
            g0 += mapping.len();
            out.push((Prob::from_log_prob(logp[i]), samples));
        }
        out
    }

    /// sample_by_profile (sample.rs:198-235) on the device (phmm_sample_reads, include/phmm_amd_generate.h): the walks
    /// 0, 1, 2, .. of profile.seed in index order, `batch` per call; a walk without bases is dropped, and under
    /// ReadLength::EmitCount a walk whose length differs (the reference's retry loop).  The random stream is the
    /// header's, not Xoshiro256PlusPlus: the reads follow the same law as the reference's, not the same bits.
    /// Unverified, like the rest of this shim: it has not been compiled here.
    pub fn sample_reads_amd(&self, profile: &SampleProfile, batch: usize) -> Historys {
        let m = AmdModel::new(self);
        let (length, kind) = match profile.length {
            ReadLength::StateCount(c) => (c, PHMM_GEN_STATE_COUNT),
            ReadLength::Endable(c) => (c, PHMM_GEN_ENDABLE),
            ReadLength::EmitCount(c) => (c, PHMM_GEN_EMIT_COUNT),
        };
        let starts: Vec<u32> = match &profile.start_points {
            StartPoints::Custom(nodes) => nodes.iter().map(|v| v.index() as u32).collect(),
            StartPoints::Random => Vec::new(),
            StartPoints::AllStartPoints => panic!("StartPoints::AllStartPoints is not resolved until sample_by_profile"),
        };
        let cap = if kind == PHMM_GEN_EMIT_COUNT { 8 * length + 65 } else { length + 1 };
        let (mut bases, mut len) = (vec![0u8; batch * (length + 1)], vec![0u32; batch]);
        let (mut hist, mut hist_len) = (vec![PHMM_PATH_NONE; batch * cap], vec![0u32; batch]);
        let mut historys = Vec::new();
        let (mut first, mut total_bases) = (0u64, 0usize);
        let more = |n: usize, b: usize| match profile.read_amount {
            ReadAmount::Count(n_reads) => n < n_reads,
            ReadAmount::TotalBases(required) => b < required,
        };
        while more(historys.len(), total_bases) {
            check(unsafe {
                phmm_sample_reads(m.0, first, batch as u64, length as u32, kind,
                                  if starts.is_empty() { ptr::null() } else { starts.as_ptr() }, starts.len() as u64,
                                  profile.seed, bases.as_mut_ptr(), len.as_mut_ptr(), ptr::null_mut(), hist.as_mut_ptr(),
                                  cap as u32, hist_len.as_mut_ptr(), ptr::null_mut())
            });
            for w in 0..batch {
                let n = len[w] as usize;
                if n == 0 || (kind == PHMM_GEN_EMIT_COUNT && n != length) {
                    continue;
                }
                let mut history = History::new();
                let mut emitted = bases[w * (length + 1)..w * (length + 1) + n].iter();
                for &code in &hist[w * cap..w * cap + hist_len[w] as usize] {
                    let state = match code {
                        PHMM_GEN_END => State::End,
                        PHMM_PATH_INS_BEGIN => State::InsBegin,
                        _ => {
                            let v = NodeIndex::new((code >> 2) as usize);
                            match code & 3 {
                                0 => State::Match(v),
                                1 => State::Ins(v),
                                _ => State::Del(v),
                            }
                        }
                    };
                    let emission = match state {
                        State::Match(_) | State::Ins(_) | State::InsBegin => Emission::Base(*emitted.next().unwrap()),
                        _ => Emission::Empty,
                    };
                    history.push(state, emission);
                }
                total_bases += n;
                historys.push(history);
                if !more(historys.len(), total_bases) {
                    break;
                }
            }
            first += batch as u64;
        }
        Historys(historys)
    }

    /// q_score_exact (q.rs:66-96) from the transition posteriors over the lists -> (init, trans, prior)
    pub fn q_score_with_mapping_amd(&self, reads: &AmdReads, mappings: &Mappings) -> (f64, f64, f64) {
        let (ef, nf) = self.to_edge_and_init_freqs_with_mapping_amd(reads, mappings);
        let m = AmdModel::new(self);
        let mut q = [0f64; 3];
        let ep = if ef.is_empty() { ptr::null() } else { ef.as_ptr() };
        check(unsafe { phmm_q_score_exact(m.0, ep, nf.as_ptr(), q.as_mut_ptr()) });
        (q[0], q[1], q[2])
    }
}

/// The cut that pays (multi_dbg/posterior.rs:483-515): ONE call per sampler iteration for all candidate
/// copy-number vectors instead of `dbg.clone(); set_copy_nums; to_phmm; to_full_prob_reads` per candidate inside a
/// rayon par_iter.  Topology, reads and mappings stay on the device for the whole k; a candidate is a row of
/// copy numbers (PHMM node id = full-edge id, multi_dbg.rs:1569-1576) and init / trans are derived on the device as
/// SeqGraph::to_phmm does (seq_graph.rs:110-135, 160-209).
pub struct AmdLikelihood {
    state: *mut phmm_likelihood,  // (first: dropped before the model, reads and mappings it borrows)
    model: AmdModel,
    reads: AmdReads,
    mappings: AmdMappings,
    n_nodes: usize,
}
impl Drop for AmdLikelihood {
    fn drop(&mut self) {
        unsafe { phmm_likelihood_destroy(self.state) }
    }
}
impl AmdLikelihood {
    pub fn new<N: PHMMNode, E: PHMMEdge, S: Seq>(phmm: &PHMMModel<N, E>, reads: &ReadCollection<S>,
                                                 mappings: &Mappings) -> AmdLikelihood {
        let model = AmdModel::new(phmm);
        let r = AmdReads::new(reads);
        let mp = AmdMappings::from_mappings(&r, mappings);
        AmdLikelihood { state: ptr::null_mut(), model, reads: r, mappings: mp, n_nodes: phmm.n_nodes() }
    }
    /// copy_nums: candidates x n_nodes, row-major -> ln P(R | X_c) per candidate (Score.likelihood, posterior.rs:259-277)
    pub fn likelihoods(&mut self, copy_nums: &[u32], min_copy_num: u32) -> Vec<Prob> {
        assert!(copy_nums.len() % self.n_nodes == 0);
        let c = copy_nums.len() / self.n_nodes;
        let mut totals = vec![0f64; c];
        check(unsafe {
            phmm_full_prob_reads_copy_nums(self.model.0, self.reads.h, self.mappings.0, c as u32, copy_nums.as_ptr(),
                                           min_copy_num, ptr::null_mut(), totals.as_mut_ptr())
        });
        totals.into_iter().map(Prob::from_log_prob).collect()
    }
    /// The same for candidates given as changes to `base` (n_nodes copy numbers): candidate c sets
    /// node[j] to cn[j] for j in off[c]..off[c+1].  Only the reads a candidate touches are run again
    /// (phmm_full_prob_reads_copy_num_changes) -> (ln P(R | X_c), reads rescored) per candidate.
    pub fn likelihoods_of_changes(&mut self, base: &[u32], off: &[u64], node: &[u32], cn: &[u32],
                                  min_copy_num: u32) -> (Vec<Prob>, Vec<u64>) {
        assert!(base.len() == self.n_nodes && !off.is_empty() && node.len() == cn.len());
        let c = off.len() - 1;
        let mut totals = vec![0f64; c];
        let mut rescored = vec![0u64; c];
        check(unsafe {
            phmm_full_prob_reads_copy_num_changes(self.model.0, self.reads.h, self.mappings.0, base.as_ptr(),
                                                  min_copy_num, c as u32, off.as_ptr(), node.as_ptr(), cn.as_ptr(),
                                                  ptr::null_mut(), totals.as_mut_ptr(), rescored.as_mut_ptr())
        });
        (totals.into_iter().map(Prob::from_log_prob).collect(), rescored)
    }

    // ---- the greedy search of sample_posterior (posterior.rs:314-417) with the sampler's state on the device
    /// Start of the search at this k: scores `copy_nums` in full once and keeps the vector and every read's ln P
    /// under it on the device (phmm_likelihood_create) -> ln P(R | X).  A second call starts over from a new vector.
    pub fn begin(&mut self, copy_nums: &[u32], min_copy_num: u32) -> Prob {
        assert!(copy_nums.len() == self.n_nodes);
        unsafe { phmm_likelihood_destroy(self.state) };
        self.state = ptr::null_mut();
        check(unsafe {
            phmm_likelihood_create(self.model.0, self.reads.h, self.mappings.0, copy_nums.as_ptr(), min_copy_num,
                                   &mut self.state)
        });
        let mut total = 0f64;
        check(unsafe { phmm_likelihood_current(self.state, ptr::null_mut(), ptr::null_mut(), &mut total) });
        Prob::from_log_prob(total)
    }
    /// sample_posterior_once (posterior.rs:470-528): the neighbours of the CURRENT vector, neighbour c sets node[j] to
    /// cn[j] for j in off[c]..off[c+1].  No base pass, no upload of the vector -> (ln P(R | X_c), reads rescored).
    pub fn likelihoods_of_neighbors(&mut self, off: &[u64], node: &[u32], cn: &[u32]) -> (Vec<Prob>, Vec<u64>) {
        assert!(!self.state.is_null() && !off.is_empty() && node.len() == cn.len());
        let c = off.len() - 1;
        let mut totals = vec![0f64; c];
        let mut rescored = vec![0u64; c];
        check(unsafe {
            phmm_likelihood_score_changes(self.state, c as u32, off.as_ptr(), node.as_ptr(), cn.as_ptr(),
                                          ptr::null_mut(), totals.as_mut_ptr(), rescored.as_mut_ptr())
        });
        (totals.into_iter().map(Prob::from_log_prob).collect(), rescored)
    }
    /// The move (posterior.rs:532-590): the current vector becomes current + changes -- one neighbour of the last
    /// batch, or the union of several independent improving moves -> ln P(R | new vector).
    pub fn accept(&mut self, node: &[u32], cn: &[u32]) -> Prob {
        assert!(!self.state.is_null() && node.len() == cn.len());
        let mut total = 0f64;
        check(unsafe {
            phmm_likelihood_move(self.state, node.len() as u64, node.as_ptr(), cn.as_ptr(), &mut total, ptr::null_mut())
        });
        Prob::from_log_prob(total)
    }
    // ---- the same search in the sampler's own units: compact edges (node groups of the handle)
    /// After begin(): group g = the k-mers of compact edge g (MultiDbg::edges_in_full; PHMM node id = full-edge id,
    /// multi_dbg.rs:1569-1576), so that neighbours and moves are stated as the sampler holds them -- copy numbers of
    /// compact edges -- and set_copy_nums' loop over every k-mer of a unitig (multi_dbg.rs:1041-1052) runs on the
    /// device.  Once per k.
    pub fn set_compact_edges(&mut self, dbg: &MultiDbg) {
        assert!(!self.state.is_null());
        let mut off: Vec<u64> = Vec::with_capacity(dbg.n_edges_compact() + 1);
        let mut nodes: Vec<u32> = Vec::with_capacity(self.n_nodes);
        off.push(0);
        for e in 0..dbg.n_edges_compact() {
            nodes.extend(dbg.edges_in_full(EdgeIndex::new(e)).iter().map(|f| f.index() as u32));
            off.push(nodes.len() as u64);
        }
        check(unsafe { phmm_likelihood_set_groups(self.state, (off.len() - 1) as u32, off.as_ptr(), nodes.as_ptr()) });
    }
    /// sample_posterior_once (posterior.rs:470-528) on the neighbours as to_neighbor_copy_nums_and_infos returns
    /// them: neighbour c changes the compact edges of its UpdateInfo cycles (neighbors.rs:193-216) to the numbers its
    /// CopyNums holds there.  No edges_in_full loop -> (ln P(R | X_c), reads rescored).
    pub fn likelihoods_of_compact_neighbors(&mut self, neighbors: &[(CopyNums, UpdateInfo)]) -> (Vec<Prob>, Vec<u64>) {
        assert!(!self.state.is_null());
        let (mut off, mut edge, mut cn) = (vec![0u64], Vec::<u32>::new(), Vec::<u32>::new());
        for (copy_nums, info) in neighbors {
            let from = edge.len();
            for cycle in &info.cycles {  // (one cycle, or the cycles of a MultiMove)
                for (e, _dir) in cycle.iter() {
                    if !edge[from..].contains(&(e.index() as u32)) {  // (a cycle may pass an edge twice)
                        edge.push(e.index() as u32);
                        cn.push(copy_nums[*e] as u32);
                    }
                }
            }
            off.push(edge.len() as u64);
        }
        let c = off.len() - 1;
        let mut totals = vec![0f64; c];
        let mut rescored = vec![0u64; c];
        check(unsafe {
            phmm_likelihood_score_group_changes(self.state, c as u32, off.as_ptr(), edge.as_ptr(), cn.as_ptr(),
                                                ptr::null_mut(), totals.as_mut_ptr(), rescored.as_mut_ptr())
        });
        (totals.into_iter().map(Prob::from_log_prob).collect(), rescored)
    }
    /// The move (posterior.rs:532-590) in compact-edge units: every k-mer of edge[j] takes cn[j] -> ln P(R | new vector).
    pub fn accept_compact(&mut self, edge: &[u32], cn: &[u32]) -> Prob {
        assert!(!self.state.is_null() && edge.len() == cn.len());
        let mut total = 0f64;
        check(unsafe {
            phmm_likelihood_move_groups(self.state, edge.len() as u64, edge.as_ptr(), cn.as_ptr(), &mut total,
                                        ptr::null_mut())
        });
        Prob::from_log_prob(total)
    }
    /// The current vector over compact edges, as get_copy_nums returns it (multi_dbg.rs:1056-1062): what a
    /// PosteriorSample.copy_nums holds.
    pub fn copy_nums_compact(&self, dbg: &MultiDbg) -> CopyNums {
        assert!(!self.state.is_null());
        let mut g = vec![0u32; dbg.n_edges_compact()];
        check(unsafe { phmm_likelihood_current_groups(self.state, g.as_mut_ptr()) });
        let mut out = CopyNums::new(g.len(), 0);
        for (e, v) in g.iter().enumerate() {
            assert!(*v != PHMM_GROUP_MIXED);  // (only a node-form accept() on part of a unitig can do that)
            out[EdgeIndex::new(e)] = *v as CopyNum;
        }
        out
    }
}
