# PGBPDevice.jl -- the reference-side binding of include/pgbp.h.
#
# What a PhyloGaussianBeliefProp.jl maintainer adds (e.g. as ext/PGBPDeviceExt.jl) so that
# calibrate!/propagate_belief!/integratebelief! run on an MI355X.  It only packs the package's own
# CanonicalBelief arrays into flat buffers, @ccall's libpgbp.so and writes results back into the SAME
# Julia arrays, so callers holding aliases (e.g. tests that read b[6] after calibrating) keep working.
# NOT exercised in the build container (no Julia there); the Python/ctypes host mirror in this
# directory's parent performs the identical call sequence and is what the test-suite drives.
module PGBPDevice

import PhyloGaussianBeliefProp as PGBP
const LIB = get(ENV, "PGBP_LIB", joinpath(@__DIR__, "..", "csrc", "libpgbp.so"))

struct Desc            # pgbp_desc
    n_clusters::Int32; n_sepsets::Int32
    dims::Ptr{Int32}; sepset_clusters::Ptr{Int32}
    scope_off::Ptr{Int64}; scope_idx::Ptr{Int32}
    n_sites::Int32; device::Int32
end
struct Opts            # pgbp_opts
    auto_stop::Int32; update_residualnorm::Int32; update_residualkldiv::Int32; reserved::Int32
    atol::Float64
end
struct Result          # pgbp_result
    succ::Int32; iscal::Int32; iter_reached::Int32; tree_reached::Int32
    fail_iter::Int32; fail_tree::Int32; fail_dir::Int32; fail_edge::Int32; fail_info::Int32; reserved::Int32
end

mutable struct DeviceClusterGraphBelief
    cgb::PGBP.ClusterGraphBelief       # the package's own object: stays the owner of the arrays
    handle::Ptr{Cvoid}
    packed::Vector{Float64}
    offsets::Vector{Int}
    schedule_set::Any
    keep::Any                          # arrays the device factor fill's static table points into
    stale::BitVector                   # lazy write-back: beliefs whose Julia arrays are older than the device's (fetch!)
    stale_residuals::Bool              # ... and the same for the message residuals as a whole (fetch_residual!)
end

check(h, rc) = rc == 0 || error(unsafe_string(@ccall LIB.pgbp_last_error(h::Ptr{Cvoid})::Cstring))

"Wrap a ClusterGraphBelief (src/clustergraphbeliefs.jl:89-109): scopeindex is evaluated once per (sepset, side)."
function DeviceClusterGraphBelief(cgb::PGBP.ClusterGraphBelief; device::Integer=0)
    b = cgb.belief; nc = cgb.nclusters; nb = length(b)
    all(x -> x isa PGBP.CanonicalBelief, b) || error("GeneralizedBelief (degenerate edges) is not supported on the device")
    dims = Int32[length(x.h) for x in b]
    sepcl = Int32[]; off = Int64[0]; idx = Int32[]
    for j in (nc+1):nb
        (l1, l2) = b[j].metadata
        for c in (cgb.cdict[l1], cgb.cdict[l2])
            push!(sepcl, c - 1)
            ind = PGBP.scopeindex(b[j], b[c])            # src/beliefs.jl:389-405, once
            append!(idx, Int32.(ind .- 1)); push!(off, off[end] + length(ind))
        end
    end
    isempty(idx) && push!(idx, 0); isempty(sepcl) && append!(sepcl, (0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve dims sepcl off idx begin
        d = Desc(nc, nb - nc, pointer(dims), pointer(sepcl), pointer(off), pointer(idx), 1, device)
        rc = @ccall LIB.pgbp_create(Ref(d)::Ref{Desc}, h::Ref{Ptr{Cvoid}})::Cint
        rc == 0 || error(unsafe_string(@ccall LIB.pgbp_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    end
    offsets = cumsum(vcat(0, [m*m + m + 1 for m in Int.(dims)]))
    obj = DeviceClusterGraphBelief(cgb, h[], zeros(offsets[end]), offsets, nothing, nothing, falses(nb), false)
    push!(obj); finalizer(o -> @ccall(LIB.pgbp_destroy(o.handle::Ptr{Cvoid})::Cvoid), obj)
    return obj
end

"host -> device: J (column-major, as stored), h, g of every belief; cluster part becomes the factors"
function Base.push!(o::DeviceClusterGraphBelief)
    for (i, x) in enumerate(o.cgb.belief)
        m = length(x.h); p = o.offsets[i]
        copyto!(o.packed, p + 1, x.J, 1, m*m); copyto!(o.packed, p + m*m + 1, x.h, 1, m); o.packed[p + m*m + m + 1] = x.g[1]
    end
    check(o.handle, @ccall LIB.pgbp_set_beliefs(o.handle::Ptr{Cvoid}, o.packed::Ptr{Float64}, 1::Int32)::Cint)
end

"""
LAZY write-back.  `calibrate!(o, ...; pull = :lazy)` moves only the result struct across the bus and marks every belief of
`o.cgb` stale; `o[j]` (= `fetch!(o, j)`) brings belief j's record over (pgbp_get_belief, a few KB) into the SAME Julia arrays
`o.cgb.belief[j].{J,h,g}` and returns that belief, so `calibrate!` followed by `integratebelief!(o, rootj)` or by reading a
handful of beliefs costs kilobytes instead of the whole state (0.76 GB at 50 000 tips x 16 traits).  `pull = :eager` (the
default, the reference's semantics for callers that read `o.cgb.belief[j]` directly) downloads everything as before.
"""
function fetch!(o::DeviceClusterGraphBelief, j::Integer)
    x = o.cgb.belief[j]
    o.stale[j] || return x
    m = length(x.h); rec = zeros(m*m + m + 1)
    check(o.handle, @ccall LIB.pgbp_get_belief(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(j - 1)::Int32, rec::Ptr{Float64})::Cint)
    copyto!(x.J, 1, rec, 1, m*m); copyto!(x.h, 1, rec, m*m + 1, m); x.g[1] = rec[m*m + m + 1]
    o.stale[j] = false
    return x
end
Base.getindex(o::DeviceClusterGraphBelief, j::Integer) = fetch!(o, j)
"the residual of the message `key = (receiver label, sender label)` (src/clustergraphbeliefs.jl:17-20), fetched alone (pgbp_get_residual)"
function fetch_residual!(o::DeviceClusterGraphBelief, key)
    mr = o.cgb.messageresidual[key]
    o.stale_residuals || return mr
    j = PGBP.sepsetindex(key[1], key[2], o.cgb); k = j - o.cgb.nclusters
    dir = o.cgb.belief[j].metadata == key ? 1 : 2          # message 2(k-1) + dir - 1 is the one received by the sepset's end `dir`
    s = length(mr.Δh); rec = zeros(max(s*s + s, 1)); flag = Ref(Int32(0)); kl = Ref(0.0); klflag = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_get_residual(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(2*(k-1) + dir - 1)::Int32,
        rec::Ptr{Float64}, flag::Ref{Int32}, kl::Ref{Float64}, klflag::Ref{Int32})::Cint)
    copyto!(mr.ΔJ, 1, rec, 1, s*s); copyto!(mr.Δh, 1, rec, s*s + 1, s)
    mr.iscalibrated_resid[1] = flag[] != 0; mr.kldiv[1] = kl[]; mr.iscalibrated_kl[1] = klflag[] != 0
    return mr
end

"device -> the SAME Julia arrays (aliases held by callers stay valid), residuals and flags included"
function pull!(o::DeviceClusterGraphBelief)
    fill!(o.stale, false); o.stale_residuals = false
    check(o.handle, @ccall LIB.pgbp_get_beliefs(o.handle::Ptr{Cvoid}, o.packed::Ptr{Float64})::Cint)
    for (i, x) in enumerate(o.cgb.belief)
        m = length(x.h); p = o.offsets[i]
        copyto!(x.J, 1, o.packed, p + 1, m*m); copyto!(x.h, 1, o.packed, p + m*m + 1, m); x.g[1] = o.packed[p + m*m + m + 1]
    end
    nm = 2 * (length(o.cgb.belief) - o.cgb.nclusters)
    rs = Int(@ccall LIB.pgbp_residual_size(o.handle::Ptr{Cvoid})::Int64)
    res = zeros(max(rs, 1)); flags = zeros(Int32, max(nm, 1)); kl = zeros(max(nm, 1)); klflags = zeros(Int32, max(nm, 1))
    check(o.handle, @ccall LIB.pgbp_get_residuals(o.handle::Ptr{Cvoid}, res::Ptr{Float64}, flags::Ptr{Int32}, kl::Ptr{Float64}, klflags::Ptr{Int32})::Cint)
    p = 0
    for (k, j) in enumerate((o.cgb.nclusters+1):length(o.cgb.belief)), (dir, key) in enumerate((o.cgb.belief[j].metadata, reverse(o.cgb.belief[j].metadata)))
        mr = o.cgb.messageresidual[key]; s = length(mr.Δh)       # key = (receiver, sender)
        copyto!(mr.ΔJ, 1, res, p + 1, s*s); copyto!(mr.Δh, 1, res, p + s*s + 1, s); p += s*s + s
        mr.iscalibrated_resid[1] = flags[2*(k-1) + dir] != 0
        mr.kldiv[1] = kl[2*(k-1) + dir]; mr.iscalibrated_kl[1] = klflags[2*(k-1) + dir] != 0   # src/beliefs.jl:895-924
    end
end

"all beliefs of one site of a batched engine (several sites sharing topology and scopes), packed like `o.packed`"
function site_beliefs(o::DeviceClusterGraphBelief, site::Integer)
    out = zeros(o.offsets[end])
    check(o.handle, @ccall LIB.pgbp_get_site_beliefs(o.handle::Ptr{Cvoid}, Int32(site - 1)::Int32, out::Ptr{Float64})::Cint)
    return out
end

# The exchange buffer of a cluster graph cut across devices (DESIGN.md section 6): the records of the listed beliefs
# (1-based, clusters then sepsets as in `o.belief`) of the first site, back to back, gathered on the device.
function pack_beliefs(o::DeviceClusterGraphBelief, beliefs::Vector{<:Integer})
    idx = Int32.(beliefs .- 1)
    n = @ccall LIB.pgbp_packed_beliefs_size(o.handle::Ptr{Cvoid}, Int32(length(idx))::Int32, idx::Ptr{Int32})::Int64
    n >= 0 || error("belief index out of range")
    buf = zeros(n)
    check(o.handle, @ccall LIB.pgbp_pack_beliefs(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(length(idx))::Int32,
                                                 idx::Ptr{Int32}, buf::Ptr{Float64})::Cint)
    return buf
end
"the reverse: overwrite the listed beliefs of the first site from a buffer another rank packed"
function unpack_beliefs!(o::DeviceClusterGraphBelief, beliefs::Vector{<:Integer}, buf::Vector{Float64})
    idx = Int32.(beliefs .- 1)
    check(o.handle, @ccall LIB.pgbp_unpack_beliefs(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(length(idx))::Int32,
                                                   idx::Ptr{Int32}, buf::Ptr{Float64})::Cint)
end
"propagate_1traversal_postorder! (dir 0) / _preorder! (dir 1) of schedule tree `tree` (1-based): the pieces a cut traversal is made of"
function traverse!(o::DeviceClusterGraphBelief, tree::Integer, dir::Integer; update_residualnorm=true)
    r = Ref(Result(ntuple(_ -> Int32(0), 10)...))
    check(o.handle, @ccall LIB.pgbp_traverse(o.handle::Ptr{Cvoid}, Int32(tree - 1)::Int32, Int32(dir)::Int32,
        Ref(Opts(0, update_residualnorm, 0, 0, 1e-5))::Ref{Opts}, r::Ref{Result})::Cint)
    return r[].succ != 0
end

function set_schedule!(o::DeviceClusterGraphBelief, schedule)
    o.schedule_set === schedule && return
    off = Int32[0]; pa = Int32[]; ch = Int32[]
    for spt in schedule                                   # (pa_lab, ch_lab, pa_j, ch_j): src/clustergraph.jl:885-894
        append!(pa, Int32.(spt[3] .- 1)); append!(ch, Int32.(spt[4] .- 1)); push!(off, length(pa))
    end
    check(o.handle, @ccall LIB.pgbp_set_schedule(o.handle::Ptr{Cvoid}, length(schedule)::Int32, off::Ptr{Int32}, pa::Ptr{Int32}, ch::Ptr{Int32})::Cint)
    o.schedule_set = schedule
end

"calibrate!(beliefs, schedule, niter; auto, info, verbose, ...) -> (succ, iscal)   (src/calibration.jl:35-60)"
function PGBP.calibrate!(o::DeviceClusterGraphBelief, schedule::AbstractVector, niter::Integer=1;
        auto::Bool=false, info::Bool=false, verbose::Bool=true,
        update_residualnorm::Bool=true, update_residualkldiv::Bool=false, pull::Symbol=:eager)
    set_schedule!(o, schedule)
    r = Ref(Result(0,0,0,0,0,0,0,0,0,0))
    check(o.handle, @ccall LIB.pgbp_calibrate(o.handle::Ptr{Cvoid}, niter::Int32,
        Ref(Opts(auto, update_residualnorm, update_residualkldiv, 0, 1e-5))::Ref{Opts}, r::Ref{Result})::Cint)
    if pull === :lazy          # nothing but `r` crosses the bus: o[j] / fetch_residual!(o, key) fetch what is read
        fill!(o.stale, true); o.stale_residuals = true
    else
        pull!(o)
    end
    res = r[]
    if res.succ == 0
        report_failure(o, schedule[res.fail_tree], res, verbose)
        info && @info "propagation failed: iteration $(res.fail_iter), schedule tree $(res.fail_tree)"
        return (false, false)
    end
    info && res.iter_reached > 0 && @info "calibration reached: iteration $(res.iter_reached), schedule tree $(res.tree_reached)"
    return (true, res.iscal != 0)
end

"integratebelief!(obj, beliefindex) -> (mu, norm)   (src/clustergraphbeliefs.jl:194)"
function PGBP.integratebelief!(o::DeviceClusterGraphBelief, j::Integer)
    m = length(o.cgb.belief[j].h); mu = zeros(max(m, 1)); norm = Ref(0.0); info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_integrate(o.handle::Ptr{Cvoid}, (j-1)::Int32, mu::Ptr{Float64}, norm::Ref{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    o.cgb.belief[j].μ[:] = mu[1:m]
    return (mu[1:m], norm[])
end

"""
    moments!(obj, beliefs = 1:nclusters; cov = true) -> Vector of (mu, Sigma, norm)

Posterior mean, covariance `inv(J)` and normalisation constant of many beliefs in one device call (pgbp_moments):
`integratebelief!` of every listed belief, bit for bit, plus the covariance the reference gets from `inv(b.J)`
(src/calibration.jl:464).  A belief that is not positive definite throws its PosDefException.
"""
function moments!(o::DeviceClusterGraphBelief, beliefs::AbstractVector{<:Integer} = 1:PGBP.nclusters(o.cgb); cov::Bool = true)
    lst = Int32.(beliefs .- 1); n = Int32(length(lst)); wc = Int32(cov)
    per = @ccall LIB.pgbp_moments_size(o.handle::Ptr{Cvoid}, n::Int32, lst::Ptr{Int32}, wc::Int32)::Int64
    per >= 0 || error("pgbp_moments: bad belief list (an index out of range, or a belief of more than 128 variables)")
    out = zeros(max(per, 1)); info = zeros(Int32, max(n, 1))
    check(o.handle, @ccall LIB.pgbp_moments(o.handle::Ptr{Cvoid}, n::Int32, lst::Ptr{Int32}, Int32(0)::Int32, Int32(1)::Int32, wc::Int32, out::Ptr{Float64}, info::Ptr{Int32})::Cint)
    res = Vector{Tuple{Vector{Float64},Union{Nothing,Matrix{Float64}},Float64}}(); at = 0
    for (i, j) in enumerate(beliefs)
        info[i] == 0 || throw(PGBP.LA.PosDefException(info[i]))
        m = length(o.cgb.belief[j].h)
        S = cov ? reshape(out[at+1:at+m*m], m, m) : nothing
        at += cov ? m * m : 0
        push!(res, (out[at+1:at+m], S, out[at+m+1])); at += m + 1
    end
    return res
end

"""
    calibrate_exact_cliquetree!(obj, spt, rootcluster, rootpos, p) -> (R_hat, mu_hat)

The sequence of `calibrate_exact_cliquetree!` (src/calibration.jl:404-517) on the device, for an engine `obj` built under the
improper root prior whose factors were assigned with R = I, mu = 0 (pgbp_lg_assignfactors): calibrate, the root's posterior
mean from `moments!`, the family sweep (pgbp_bm_exact_stats), `R_hat = num / den`.  The score of the returned fixed-root
model is one `pgbp_lg_assignfactors` + log-likelihood evaluation on a second engine built with a fixed root (the reference
re-allocates the root's scope in place, :507-511).
"""
function calibrate_exact_cliquetree!(o::DeviceClusterGraphBelief, spt, rootcluster::Integer, rootpos::Integer, p::Integer)
    PGBP.calibrate!(o, [spt])
    mu, _, _ = moments!(o, [rootcluster]; cov = false)[1]
    num = zeros(p * p); den = Ref(0.0); info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_bm_exact_stats(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, num::Ptr{Float64}, den::Ref{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (reshape(num, p, p) ./ den[], mu[rootpos:rootpos+p-1])
end

"""
    lg_gradient(obj, p, nrates; ou = false) -> (dR, dmu, dalpha, dtheta)

The exact gradient of the log-likelihood with respect to the parameters of the last pgbp_lg_assignfactors, from the current
beliefs (pgbp_lg_gradient: Fisher's identity, one sweep over the node families).  Exact only when the beliefs are calibrated
(postorder and preorder) on a clique tree under those parameters; on a loopy graph, at a converged calibration, the gradient of
the factored energy.  `dR[:, :, c]` is symmetric with d loglik = tr(dR[:, :, c] * dR_c); dalpha, dtheta are zero unless `ou`.
"""
function lg_gradient(o::DeviceClusterGraphBelief, p::Integer, nrates::Integer; ou::Bool = false)
    dR = zeros(p * p * nrates); dmu = zeros(p); dalpha = Ref(0.0); dtheta = zeros(p); info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_lg_gradient(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, dR::Ptr{Float64}, dmu::Ptr{Float64}, dalpha::Ref{Float64}, dtheta::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (reshape(dR, p, p, nrates), dmu, dalpha[], dtheta)
end

"""
    lg_gradient_sites(obj, nsites, nrates; noise = false) -> (dR, dmu, dalpha, dtheta, dsigma_e, info)

`lg_gradient` for every site of a univariate batch on the thread-per-site kernels (pgbp_lg_gradient_sites: p = 1, every belief
of at most 2 variables, at least 8 sites), lanes = sites; the beliefs are read in the layout they are in.  `dR[c, s]` is rate c
of site s, the others one number per site (`dsigma_e` is `nothing` unless `noise`).  `info[s] != 0` marks a site whose cluster
`info[s]` is not positive definite: its outputs are NaN, no exception is thrown.
"""
function lg_gradient_sites(o::DeviceClusterGraphBelief, nsites::Integer, nrates::Integer; noise::Bool = false)
    dR = zeros(nrates, nsites); dmu = zeros(nsites); dalpha = zeros(nsites); dtheta = zeros(nsites)
    dsig = noise ? zeros(nsites) : nothing
    info = zeros(Int32, nsites)
    check(o.handle, @ccall LIB.pgbp_lg_gradient_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, dR::Ptr{Float64}, dmu::Ptr{Float64}, dalpha::Ptr{Float64}, dtheta::Ptr{Float64}, (noise ? pointer(dsig) : Ptr{Float64}(C_NULL))::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (dR, dmu, dalpha, dtheta, dsig, info)
end

"""
    lg_shift_scan_sites(obj, nsites, nfamilies; min_info = 1e-8, information = false, tables = true)
        -> (jump, lr, H, top_lr, top_family, info)

The scan of every edge for a mean shift for every site of a univariate batch on the thread-per-site kernels
(pgbp_lg_shift_scan_sites; the conditions of `lg_gradient_sites`), lanes = sites, nothing converted.  `jump[s, f]`, `lr[s, f]` and
`H[s, f]` (with `information`) are the call's site-minor rows; `top_lr[s]` and `top_family[s]` (1-based, 0: nothing identified
or a failed site) the largest lr of a site and its family, formed on the device.  `tables = false` fetches no table (`nothing`).
"""
function lg_shift_scan_sites(o::DeviceClusterGraphBelief, nsites::Integer, nfamilies::Integer; min_info::Real = 1e-8,
                             information::Bool = false, tables::Bool = true)
    jump = tables ? zeros(nsites, nfamilies) : nothing
    lr = tables ? zeros(nsites, nfamilies) : nothing
    H = (tables && information) ? zeros(nsites, nfamilies) : nothing
    top = zeros(nsites); topf = zeros(Int32, nsites); info = zeros(Int32, nsites)
    ptr(x) = x === nothing ? Ptr{Float64}(C_NULL) : pointer(x)
    GC.@preserve jump lr H check(o.handle, @ccall LIB.pgbp_lg_shift_scan_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, Float64(min_info)::Float64, ptr(jump)::Ptr{Float64}, ptr(lr)::Ptr{Float64}, ptr(H)::Ptr{Float64}, top::Ptr{Float64}, topf::Ptr{Int32}, info::Ptr{Int32})::Cint)
    return (jump, lr, H, top, Int.(topf) .+ 1, info)
end

"""
    lg_optimum_scan_sites(obj, nsites, nfamilies; min_info = 1e-8, information = false, tables = true)
        -> (delta, lr, H, top_lr, top_family, info)

The scan of every edge for a shift of the optimum of its clade under OU, for every site of a univariate batch on a tree on the
thread-per-site kernels (pgbp_lg_optimum_scan_sites; the conditions of `lg_gradient_sites`, a topology set, one parent per
family), lanes = sites, nothing converted.  The painted optima in force are read: the scan gives the increment.  `delta[s, f]`,
`lr[s, f]` and `H[s, f]` (with `information`; se = 1 / sqrt(H)) are the call's site-minor rows; `top_lr[s]` and `top_family[s]`
(1-based, 0: nothing identified or a failed site) the largest lr of a site and its family, formed on the device.
`tables = false` fetches no table (`nothing`).  Written, not yet run.
"""
function lg_optimum_scan_sites(o::DeviceClusterGraphBelief, nsites::Integer, nfamilies::Integer; min_info::Real = 1e-8,
                               information::Bool = false, tables::Bool = true)
    delta = tables ? zeros(nsites, nfamilies) : nothing
    lr = tables ? zeros(nsites, nfamilies) : nothing
    H = (tables && information) ? zeros(nsites, nfamilies) : nothing
    top = zeros(nsites); topf = zeros(Int32, nsites); info = zeros(Int32, nsites)
    ptr(x) = x === nothing ? Ptr{Float64}(C_NULL) : pointer(x)
    GC.@preserve delta lr H check(o.handle, @ccall LIB.pgbp_lg_optimum_scan_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, Float64(min_info)::Float64, ptr(delta)::Ptr{Float64}, ptr(lr)::Ptr{Float64}, ptr(H)::Ptr{Float64}, top::Ptr{Float64}, topf::Ptr{Int32}, info::Ptr{Int32})::Cint)
    return (delta, lr, H, top, Int.(topf) .+ 1, info)
end

"""
    lg_set_clade_shifts_sites!(obj, family, delta)
    lg_update_clade_shifts_sites!(obj, delta)
    lg_clear_clade_shifts_sites!(obj)
    lg_clade_shift_slots(obj) -> Int
    lg_clade_shift_score_sites(obj, nsites; min_info = 1e-8) -> (g, H, Kt, info)

Per-site clade shifts of the OU optimum on a thread-per-site engine with a topology set (pgbp_lg_set_clade_shifts_sites and its
companions): at site `s` the optimum of every edge of clade(`family[s, j]`) gains `delta[s, j]`.  `family` is `nsites x nslots`
with 1-based families and 0 for an empty slot (Julia's column-major `[site, slot]` is the call's `[slot][site]`); `delta` has the
same shape.  The setting takes effect at the next fill; `lg_optimum_scan_sites` honours it, the gradient calls refuse while it
is in force.  `lg_update_clade_shifts_sites!` replaces the deltas alone.  The score call returns, per slot and site, the scan's
g, H and Kt at the site's own family (`nsites x nslots`; NaN at an empty slot, H NaN where the slot is not identified).
Written, not yet run.
"""
function lg_set_clade_shifts_sites!(o::DeviceClusterGraphBelief, family::AbstractMatrix{<:Integer}, delta::AbstractMatrix{<:Real})
    size(family) == size(delta) || throw(ArgumentError("family and delta differ in shape"))
    fam = Matrix{Int32}(family .- 1)
    d = Matrix{Float64}(delta)
    check(o.handle, @ccall LIB.pgbp_lg_set_clade_shifts_sites(o.handle::Ptr{Cvoid}, Int32(size(fam, 2))::Int32, fam::Ptr{Int32}, d::Ptr{Float64})::Cint)
    return o
end

function lg_update_clade_shifts_sites!(o::DeviceClusterGraphBelief, delta::AbstractMatrix{<:Real})
    d = Matrix{Float64}(delta)
    check(o.handle, @ccall LIB.pgbp_lg_update_clade_shifts_sites(o.handle::Ptr{Cvoid}, d::Ptr{Float64})::Cint)
    return o
end

function lg_clear_clade_shifts_sites!(o::DeviceClusterGraphBelief)
    check(o.handle, @ccall LIB.pgbp_lg_set_clade_shifts_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64})::Cint)
    return o
end

lg_clade_shift_slots(o::DeviceClusterGraphBelief) = Int(@ccall LIB.pgbp_lg_clade_shift_slots(o.handle::Ptr{Cvoid})::Int32)

function lg_clade_shift_score_sites(o::DeviceClusterGraphBelief, nsites::Integer; min_info::Real = 1e-8)
    m = lg_clade_shift_slots(o)
    g = zeros(nsites, m); H = zeros(nsites, m); kt = zeros(nsites, m); info = zeros(Int32, nsites)
    check(o.handle, @ccall LIB.pgbp_lg_clade_shift_score_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, Float64(min_info)::Float64, g::Ptr{Float64}, H::Ptr{Float64}, kt::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (g, H, kt, info)
end

"""
    lg_edge_gradient_sites(obj, nsites, nfamilies, K) -> (dlength, dgamma, dshift, info)

`lg_edge_gradient` for every site of a univariate batch on the thread-per-site kernels (pgbp_lg_edge_gradient_sites), lanes =
sites: `dlength[s, k, f]`, `dgamma[s, k, f]`, `dshift[s, f]`; a failed site (`info[s] != 0`) holds NaN.
"""
function lg_edge_gradient_sites(o::DeviceClusterGraphBelief, nsites::Integer, nfamilies::Integer, K::Integer)
    dlength = zeros(nsites, K, nfamilies); dgamma = zeros(nsites, K, nfamilies); dshift = zeros(nsites, nfamilies)
    info = zeros(Int32, nsites)
    check(o.handle, @ccall LIB.pgbp_lg_edge_gradient_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, dlength::Ptr{Float64}, dgamma::Ptr{Float64}, dshift::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (dlength, dgamma, dshift, info)
end

"""
    lg_loo_sites(obj, nsites) -> (mean, var, lpd, total, info)

`lg_loo` for every site of a univariate batch on the thread-per-site kernels (pgbp_lg_loo_sites), lanes = sites, for the tip
families of `lg_loo_families` in that order: `mean[s, t]`, `var[s, t]`, `lpd[s, t]`, `info[s, t]` and `total[s]` (NaN where a
tip of the site is not determined).
"""
function lg_loo_sites(o::DeviceClusterGraphBelief, nsites::Integer)
    nt = max(length(lg_loo_families(o)), 1)
    mean = zeros(nsites, nt); var = zeros(nsites, nt); lpd = zeros(nsites, nt); total = zeros(nsites)
    info = zeros(Int32, nsites, nt)
    check(o.handle, @ccall LIB.pgbp_lg_loo_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, mean::Ptr{Float64}, var::Ptr{Float64}, lpd::Ptr{Float64}, total::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (mean, var, lpd, total, info)
end

"""
    bm_exact_stats_sites(obj, nsites, rootcluster, rootpos) -> (num, den, mu, info)

The family sweep of `calibrate_exact_cliquetree!` for every site of a univariate batch on the thread-per-site kernels
(pgbp_bm_exact_stats_sites), lanes = sites, with the per-site mask of missing tips and the shifts in force: `num[s]`, `den[s]`
(the number of tips site `s` observes less one, to rounding; `num ./ den` is the REML rate) and `mu[s]`, the posterior mean of
variable `rootpos` of cluster `rootcluster` (both 1-based).  The beliefs must be calibrated under a BM with R = 1 and an improper
root.  A failed site (`info[s] != 0`) holds NaN.  Untested: there is no Julia on the test machines.
"""
function bm_exact_stats_sites(o::DeviceClusterGraphBelief, nsites::Integer, rootcluster::Integer, rootpos::Integer)
    num = zeros(nsites); den = zeros(nsites); mu = zeros(nsites); info = zeros(Int32, nsites)
    check(o.handle, @ccall LIB.pgbp_bm_exact_stats_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, Int32(rootcluster - 1)::Int32, Int32(rootpos - 1)::Int32, num::Ptr{Float64}, den::Ptr{Float64}, mu::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (num, den, mu, info)
end

"""
    bm_rate_matrix_sites(obj, rows, cols, rootcluster, rootpos) -> (gram, den, mu, info)

The evolutionary rate matrix between the sites of a univariate batch on the thread-per-site kernels
(pgbp_bm_rate_matrix_sites): `gram[a, b] = (Y'PY)_ab` for the sites `rows` against the sites `cols` (1-based unit ranges),
formed on the matrix cores; `den`, `mu`, `info`: the values of `bm_exact_stats_sites` for the row sites, then for the column
sites.  `gram ./ sqrt.(den_rows * den_cols')` is the REML rate matrix.  The beliefs must be calibrated under a BM with R = 1
and an improper root, and every site must observe the same tips (a per-site mask is refused).  A failed site holds NaN in its
row or column.  Untested: there is no Julia on the test machines.
"""
function bm_rate_matrix_sites(o::DeviceClusterGraphBelief, rows::UnitRange{<:Integer}, cols::UnitRange{<:Integer}, rootcluster::Integer, rootpos::Integer)
    nr = length(rows); nc = length(cols)
    g = zeros(nc, nr)   # (the call writes row-major [rows][cols]: column-major [cols, rows])
    den = zeros(nr + nc); mu = zeros(nr + nc); info = zeros(Int32, nr + nc)
    check(o.handle, @ccall LIB.pgbp_bm_rate_matrix_sites(o.handle::Ptr{Cvoid}, Int32(first(rows) - 1)::Int32, Int32(last(rows))::Int32, Int32(first(cols) - 1)::Int32, Int32(last(cols))::Int32, Int32(rootcluster - 1)::Int32, Int32(rootpos - 1)::Int32, g::Ptr{Float64}, den::Ptr{Float64}, mu::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (permutedims(g), den, mu, info)
end

"""
    bm_rate_apply_sites(obj, V, sites, rootcluster, rootpos) -> (GV, den, mu, info)

The rate matrix of `bm_rate_matrix_sites(obj, sites, sites, ...)` applied to the columns of `V` (`length(sites)` x k) without
the matrix being formed (pgbp_bm_rate_apply_sites): `GV = gram * V`, two skinny products with the residual rows on the matrix
cores, for iterative consumers (leading principal components, solves, trace estimates).  `V` travels in calls of at most 64
columns; `den`, `mu`, `info`: as `bm_exact_stats_sites` over `sites` (a 1-based unit range).  If any site has `info != 0`, `GV`
is NaN in every entry: check `info` once.  Untested: there is no Julia on the test machines.
"""
function bm_rate_apply_sites(o::DeviceClusterGraphBelief, V::AbstractMatrix{<:Real}, sites::UnitRange{<:Integer}, rootcluster::Integer, rootpos::Integer)
    n = length(sites); k = size(V, 2)
    size(V, 1) == n || throw(DimensionMismatch("V has $(size(V, 1)) rows; the range holds $n sites"))
    GV = zeros(n, k)
    den = zeros(n); mu = zeros(n); info = zeros(Int32, n)
    for j0 in 1:64:max(k, 1)
        j1 = min(k, j0 + 63)
        v = Matrix{Float64}(V[:, j0:j1])   # (column-major [sites, vectors] is the call's [n_vec][sites], site-minor)
        gv = zeros(n, j1 - j0 + 1)
        check(o.handle, @ccall LIB.pgbp_bm_rate_apply_sites(o.handle::Ptr{Cvoid}, Int32(first(sites) - 1)::Int32, Int32(last(sites))::Int32, Int32(j1 - j0 + 1)::Int32, v::Ptr{Float64}, Int32(rootcluster - 1)::Int32, Int32(rootpos - 1)::Int32, gv::Ptr{Float64}, den::Ptr{Float64}, mu::Ptr{Float64}, info::Ptr{Int32})::Cint)
        GV[:, j0:j1] = gv
    end
    return (GV, den, mu, info)
end

"""
    moments_sites(obj, nsites, dims; cov = true) -> (mean, tri, norm, info)

`moments!` of EVERY CLUSTER for every site of a univariate batch on the thread-per-site kernels (pgbp_moments_sites; the
conditions of `lg_gradient_sites`), lanes = sites, nothing converted.  `dims`: the clusters' dimensions (0, 1 or 2).  The
call's site-minor rows: `mean[s, i]` over the clusters' variables, cluster after cluster; `tri[s, i]` the packed upper triangle
of Sigma = J^-1 per cluster (S00, S01, S11; `nothing` without `cov`); `norm[s, c]`, `info[s, c]` (0, or PosDefException.info:
that cluster's entries are NaN).  Untested: there is no Julia on the test machines.
"""
function moments_sites(o::DeviceClusterGraphBelief, nsites::Integer, dims::AbstractVector{<:Integer}; cov::Bool = true)
    nc = length(dims)
    mean = zeros(nsites, max(sum(dims), 1))
    tri = cov ? zeros(nsites, max(sum(m * (m + 1) ÷ 2 for m in dims), 1)) : nothing
    norm = zeros(nsites, max(nc, 1)); info = zeros(Int32, nsites, max(nc, 1))
    GC.@preserve tri check(o.handle, @ccall LIB.pgbp_moments_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Ptr{Int32}(C_NULL)::Ptr{Int32}, Int32(0)::Int32, Int32(nsites)::Int32, mean::Ptr{Float64}, (cov ? pointer(tri) : Ptr{Float64}(C_NULL))::Ptr{Float64}, norm::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (mean, tri, norm, info)
end

"""
    sample_posterior_sites(obj, nsites, ndraws = 1; z = nothing, seed = 0, tree = 1) -> (x, info)

`sample_posterior!` for every site of a univariate batch on the thread-per-site kernels (pgbp_sample_posterior_sites), lanes =
sites: `x[s, i, d]` = entry `i` of draw `d` at site `s` (the entry layout of `sample_posterior!`, transposed); `z` the same
shape, or `nothing`: the device generates the normals from `seed` (Philox4x32-10, the convention of include/pgbp.h).
`info[s]`: 0, or the 1-based index of the first cluster in preorder whose conditional precision is not positive definite
(that site's draws are NaN).  `tree`: 1-based index into the schedule that was set.  Untested: no Julia on the test machines.
"""
function sample_posterior_sites(o::DeviceClusterGraphBelief, nsites::Integer, ndraws::Integer = 1;
                                z::Union{Nothing,Array{Float64,3}} = nothing, seed::Integer = 0, tree::Integer = 1)
    size = sample_size(o)
    z === nothing || Base.size(z) == (nsites, size, ndraws) || error("z has size $(Base.size(z)), expected $((nsites, size, ndraws))")
    x = zeros(nsites, max(size, 1), max(ndraws, 1)); info = zeros(Int32, nsites)
    GC.@preserve z check(o.handle, @ccall LIB.pgbp_sample_posterior_sites(o.handle::Ptr{Cvoid}, Int32(tree - 1)::Int32, Int32(0)::Int32, Int32(nsites)::Int32, Int32(ndraws)::Int32, (z === nothing ? Ptr{Float64}(C_NULL) : pointer(z))::Ptr{Float64}, UInt64(seed)::UInt64, x::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (x, info)
end

"""
    posterior_cov_sites(obj, nsites, c; tree = 1, want_w = true, want_k = true, want_gram = true) -> (w, k, gram, info)

`posterior_cov` for every site of a univariate batch on the thread-per-site kernels (pgbp_posterior_cov_sites), lanes = sites.
`c[i, a]`: the weight of column `a` on entry `i` of `sample_posterior!`'s layout, shared by the sites.  `w[s, i, a]` = A'c and
`k[s, i, a]` = Cov(x_i, c_a'x | data) at site `s`; `gram[s, q]`, `q` over the upper triangle in column order (G00, G01, G11,
...), = Cov(c_a'x, c_b'x | data), folded on the device -- with `gram` alone no table of size x sites is moved.  An output that
is not wanted is `nothing`.  `info[s]`: 0, or the 1-based index of the first cluster in preorder whose conditional precision is
not positive definite (that site is NaN).  `tree`: 1-based index into the schedule that was set.  Untested: no Julia on the test
machines.
"""
function posterior_cov_sites(o::DeviceClusterGraphBelief, nsites::Integer, c::Matrix{Float64}; tree::Integer = 1,
                             want_w::Bool = true, want_k::Bool = true, want_gram::Bool = true)
    size = sample_size(o)
    Base.size(c, 1) == size || error("c has $(Base.size(c, 1)) rows, expected $size")
    ncols = Base.size(c, 2)
    w = want_w ? zeros(nsites, max(size, 1), max(ncols, 1)) : nothing
    k = want_k ? zeros(nsites, max(size, 1), max(ncols, 1)) : nothing
    gram = want_gram ? zeros(nsites, max(ncols * (ncols + 1) ÷ 2, 1)) : nothing
    info = zeros(Int32, nsites)
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve w k gram check(o.handle, @ccall LIB.pgbp_posterior_cov_sites(o.handle::Ptr{Cvoid}, Int32(tree - 1)::Int32, Int32(0)::Int32, Int32(nsites)::Int32, Int32(ncols)::Int32, c::Ptr{Float64}, ptr(w)::Ptr{Float64}, ptr(k)::Ptr{Float64}, ptr(gram)::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (w, k, gram, info)
end

"""
    lg_impute_sites(obj, nsites) -> (mean, var, info)

`lg_impute` for every site of a univariate batch on the thread-per-site kernels (pgbp_lg_impute_sites), lanes = sites, for the
families of `lg_impute_families` in that order: `mean[s, t]`, `var[s, t]` (NaN where nothing is predicted) and `info[s, t]`
(the codes of `lg_impute`).  Untested: no Julia on the test machines.
"""
function lg_impute_sites(o::DeviceClusterGraphBelief, nsites::Integer)
    n = @ccall LIB.pgbp_lg_impute_count(o.handle::Ptr{Cvoid})::Int32
    n >= 0 || error("pgbp_lg_impute_count: no family table (call pgbp_lg_setup first)")
    nt = max(Int(n), 1)
    mean = fill(NaN, nsites, nt); var = fill(NaN, nsites, nt); info = zeros(Int32, nsites, nt)
    check(o.handle, @ccall LIB.pgbp_lg_impute_sites(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, mean::Ptr{Float64}, var::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (mean[:, 1:n], var[:, 1:n], info[:, 1:n])
end

"""
    lg_loo_families(obj) -> Vector{Int}

The tip families of the table given to pgbp_lg_setup (1-based indices into it), in the order of `lg_loo`'s outputs
(pgbp_lg_loo_count, pgbp_lg_loo_families).
"""
function lg_loo_families(o::DeviceClusterGraphBelief)
    n = @ccall LIB.pgbp_lg_loo_count(o.handle::Ptr{Cvoid})::Int32
    n >= 0 || error("pgbp_lg_loo_count: no family table (call pgbp_lg_setup first)")
    fam = zeros(Int32, max(n, 1))
    check(o.handle, @ccall LIB.pgbp_lg_loo_families(o.handle::Ptr{Cvoid}, fam::Ptr{Int32})::Cint)
    return Int.(fam[1:n]) .+ 1
end

"""
    lg_loo(obj, p) -> (mean, cov, lpd, total, info)

Leave-one-out predictive moments of every tip with data, given the data of all other tips, from the current beliefs
(pgbp_lg_loo: one sweep over the tip families).  Exact only when the beliefs are calibrated (postorder and preorder) on a clique
tree under the parameters of the last pgbp_lg_assignfactors; on a loopy graph, at a converged calibration, the Bethe
approximation.  `mean[:, i]` and `cov[:, :, i]` of tip family i (`lg_loo_families`) are NaN at its unobserved traits; `lpd[i]` is
the log predictive density of its observed values, `total` their sum; `info[i]` is 0, 1 when the other data do not determine
the prediction, or 1 + PosDefException.info of the cluster (that tip's values are NaN; nothing is thrown).
"""
function lg_loo(o::DeviceClusterGraphBelief, p::Integer)
    n = length(lg_loo_families(o))
    mean = zeros(p, max(n, 1)); cov = zeros(p, p, max(n, 1)); lpd = zeros(max(n, 1)); total = Ref(0.0)
    info = zeros(Int32, max(n, 1))
    check(o.handle, @ccall LIB.pgbp_lg_loo(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, mean::Ptr{Float64}, cov::Ptr{Float64}, lpd::Ptr{Float64}, total::Ref{Float64}, info::Ptr{Int32})::Cint)
    return (mean[:, 1:n], cov[:, :, 1:n], lpd[1:n], total[], info[1:n])
end

"""
    lg_impute_families(obj) -> (families::Vector{Int}, predicted::Vector{UInt64})

The tip families of the table given to pgbp_lg_setup that miss a trait (1-based indices into it), in the order of `lg_impute`'s
outputs, and per family the mask of the traits that are predicted (bit t-1 = trait t): the missing traits that every parent in a
cluster holds in scope (pgbp_lg_impute_count, pgbp_lg_impute_families).
"""
function lg_impute_families(o::DeviceClusterGraphBelief)
    n = @ccall LIB.pgbp_lg_impute_count(o.handle::Ptr{Cvoid})::Int32
    n >= 0 || error("pgbp_lg_impute_count: no family table (call pgbp_lg_setup first)")
    fam = zeros(Int32, max(n, 1)); pred = zeros(UInt64, max(n, 1))
    check(o.handle, @ccall LIB.pgbp_lg_impute_families(o.handle::Ptr{Cvoid}, fam::Ptr{Int32}, pred::Ptr{UInt64})::Cint)
    return (Int.(fam[1:n]) .+ 1, pred[1:n])
end

"""
    lg_impute(obj, p) -> (mean, cov, info)

Posterior moments of the missing values of every tip, given all the data, from the current beliefs (pgbp_lg_impute: one sweep
over the tip families that miss a trait).  Exact under the condition of `lg_loo`.  `mean[:, i]` and `cov[:, :, i]` of listed
family i (`lg_impute_families`) are NaN outside its predicted traits; `info[i]` is 0, -1 when nothing of the tip is predicted, 1
when its variance is not positive definite, or 1 + PosDefException.info of the cluster (that tip's values are NaN; nothing is
thrown).  `pgbp_impute_scratch_limit` bounds the device copies of the outputs, as `pgbp_loo_scratch_limit` does.
"""
function lg_impute(o::DeviceClusterGraphBelief, p::Integer)
    n = length(lg_impute_families(o)[1])
    mean = fill(NaN, p, max(n, 1)); cov = fill(NaN, p, p, max(n, 1)); info = zeros(Int32, max(n, 1))
    check(o.handle, @ccall LIB.pgbp_lg_impute(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, mean::Ptr{Float64}, cov::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (mean[:, 1:n], cov[:, :, 1:n], info[1:n])
end

impute_scratch_limit(doubles::Integer) = @ccall LIB.pgbp_impute_scratch_limit(Int64(doubles)::Int64)::Cvoid

"""
    lg_edge_gradient(obj, p, nfamilies, K) -> (dlength, dgamma, dshift)

Derivatives of the log-likelihood in every edge from the current beliefs (pgbp_lg_edge_gradient: one sweep over the node
families, each writing its own numbers): `dlength[k, f]` and `dgamma[k, f]` for parent edge k of family f of the table given to
pgbp_lg_setup (`K` = its max_parents; NaN where the family has no such edge; `dgamma` is the free partial in each inheritance:
with gamma_minor = 1 - gamma_major the derivative in gamma_major is `dgamma[major] - dgamma[minor]`), `dshift[:, f]` the score of
an additive shift of the child's conditional mean (a root-prior family: its dmu term).  Exact under the condition of
`lg_gradient`.  A cluster that is not positive definite throws its PosDefException.
"""
function lg_edge_gradient(o::DeviceClusterGraphBelief, p::Integer, nfamilies::Integer, K::Integer)
    dlength = zeros(K, max(nfamilies, 1)); dgamma = zeros(K, max(nfamilies, 1)); dshift = zeros(p, max(nfamilies, 1))
    info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_lg_edge_gradient(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, dlength::Ptr{Float64}, dgamma::Ptr{Float64}, dshift::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (dlength[:, 1:nfamilies], dgamma[:, 1:nfamilies], dshift[:, 1:nfamilies])
end

"""
    lg_set_edges!(obj; length = nothing, gamma = nothing)

New edge lengths and / or inheritances for the family table given to pgbp_lg_setup (pgbp_lg_set_edges): `K x nfamilies`
matrices (or vectors in that order), `nothing` leaves the values as they are.  The next pgbp_lg_assignfactors or
pgbp_enqueue_loglik_lg uses them; a length that is not positive and finite is an error and nothing changes.
"""
function lg_set_edges!(o::DeviceClusterGraphBelief; length::Union{Nothing,AbstractArray{Float64}} = nothing,
                       gamma::Union{Nothing,AbstractArray{Float64}} = nothing)
    len = length === nothing ? C_NULL : Array{Float64}(length)   # (the call keeps what it converts alive)
    gam = gamma === nothing ? C_NULL : Array{Float64}(gamma)
    check(o.handle, @ccall LIB.pgbp_lg_set_edges(o.handle::Ptr{Cvoid}, len::Ptr{Float64}, gam::Ptr{Float64})::Cint)
    return nothing
end

"""
    lg_set_shifts!(obj, edges, values)

Mean shifts on edges (pgbp_lg_set_shifts): `edges` holds the 0-based indices `f * K + k` of the family table given to
pgbp_lg_setup (family `f`, parent edge `k`, `K` = max_parents), `values` is `p x length(edges)` (one shift per column) or
`p x length(edges) x n_sites` for one set per site.  The child's conditional mean gains `sum_k gamma_k s_k`.  An empty
`edges` clears the shifts; the call replaces the previous list.  The next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg
uses them; an invalid entry is an error and nothing changes.
"""
function lg_set_shifts!(o::DeviceClusterGraphBelief, edges::AbstractVector{<:Integer}, values::AbstractArray{Float64})
    ed = Vector{Int32}(edges)
    val = Array{Float64}(values)
    per_site = ndims(val) == 3 ? Int32(1) : Int32(0)
    check(o.handle, @ccall LIB.pgbp_lg_set_shifts(o.handle::Ptr{Cvoid}, Int32(Base.length(ed))::Int32, ed::Ptr{Int32},
                                                  val::Ptr{Float64}, per_site::Int32)::Cint)
    return nothing
end

"""
    lg_shift_count(obj) -> Int

Number of mean shifts in force (pgbp_lg_shift_count): 0 when none is set, -1 without a family table.
"""
lg_shift_count(o::DeviceClusterGraphBelief) = Int(@ccall LIB.pgbp_lg_shift_count(o.handle::Ptr{Cvoid})::Int32)

"""
    lg_set_optima!(obj, regime, values)

Painted optima under OU (pgbp_lg_set_optima): `regime` holds one integer per entry `f * K + k` of the family table given to
pgbp_lg_setup (`K x n_families` as a matrix; 0: the edge keeps `theta`, `r >= 1`: its optimum is column `r` of `values`),
`values` is `p x n_regimes`, or `p x n_regimes x n_sites` for one set per site.  The offset of a family becomes
`sum_k wc_k theta_{r(f,k)}`; under BM nothing changes.  An empty `values` clears the optima; the call replaces the previous
setting and takes effect at the next fill; an invalid entry is an error and nothing changes.  `lg_gradient_optima` and
`lg_gradient_sites_optima` return the derivative in every optimum; the other sweeps that form the offsets refuse under OU while
optima are in force.
"""
function lg_set_optima!(o::DeviceClusterGraphBelief, regime::AbstractArray{<:Integer}, values::AbstractArray{Float64})
    reg = Vector{Int32}(vec(regime))
    val = Array{Float64}(values)
    per_site = ndims(val) == 3 ? Int32(1) : Int32(0)
    n = isempty(val) ? Int32(0) : Int32(size(val, 2))
    check(o.handle, @ccall LIB.pgbp_lg_set_optima(o.handle::Ptr{Cvoid}, n::Int32, reg::Ptr{Int32}, val::Ptr{Float64},
                                                  per_site::Int32)::Cint)
    return nothing
end

"""
    lg_update_optima!(obj, values)

New values for the optima in force (pgbp_lg_update_optima), in the shape `lg_set_optima!` was given; the regime map stays.
"""
function lg_update_optima!(o::DeviceClusterGraphBelief, values::AbstractArray{Float64})
    val = Array{Float64}(values)
    check(o.handle, @ccall LIB.pgbp_lg_update_optima(o.handle::Ptr{Cvoid}, val::Ptr{Float64})::Cint)
    return nothing
end

"""
    lg_optima_count(obj) -> Int

Number of regimes in force (pgbp_lg_optima_count): 0 when none is set, -1 without a family table.
"""
lg_optima_count(o::DeviceClusterGraphBelief) = Int(@ccall LIB.pgbp_lg_optima_count(o.handle::Ptr{Cvoid})::Int32)

"""
    lg_gradient_optima(obj, p, nrates, nregimes; noise = false) -> (dR, dmu, dalpha, dtheta, dsigma_e, doptima)

`lg_gradient` of the current site with painted optima in force (pgbp_lg_gradient_optima): `doptima` is `p x nregimes`, `dtheta`
the derivative in the optimum of the unpainted edges, `dsigma_e` `nothing` unless `noise`.
"""
function lg_gradient_optima(o::DeviceClusterGraphBelief, p::Integer, nrates::Integer, nregimes::Integer; noise::Bool = false)
    dR = zeros(p * p * nrates); dmu = zeros(p); dalpha = Ref(0.0); dtheta = zeros(p); info = Ref(Int32(0))
    dsig = noise ? zeros(p, p) : nothing
    dopt = zeros(p, nregimes)
    GC.@preserve dsig check(o.handle, @ccall LIB.pgbp_lg_gradient_optima(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, dR::Ptr{Float64}, dmu::Ptr{Float64}, dalpha::Ref{Float64}, dtheta::Ptr{Float64}, (noise ? pointer(dsig) : Ptr{Float64}(C_NULL))::Ptr{Float64}, dopt::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (reshape(dR, p, p, nrates), dmu, dalpha[], dtheta, dsig, dopt)
end

"""
    lg_gradient_sites_optima(obj, nsites, nrates, nregimes; noise = false) -> (dR, dmu, dalpha, dtheta, dsigma_e, doptima, info)

`lg_gradient_sites` with painted optima in force (pgbp_lg_gradient_sites_optima): `doptima[r, s]` is the derivative of site s in
the optimum of regime r.
"""
function lg_gradient_sites_optima(o::DeviceClusterGraphBelief, nsites::Integer, nrates::Integer, nregimes::Integer; noise::Bool = false)
    dR = zeros(nrates, nsites); dmu = zeros(nsites); dalpha = zeros(nsites); dtheta = zeros(nsites)
    dsig = noise ? zeros(nsites) : nothing
    dopt = zeros(nregimes, nsites)
    info = zeros(Int32, nsites)
    GC.@preserve dsig check(o.handle, @ccall LIB.pgbp_lg_gradient_sites_optima(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(nsites)::Int32, dR::Ptr{Float64}, dmu::Ptr{Float64}, dalpha::Ptr{Float64}, dtheta::Ptr{Float64}, (noise ? pointer(dsig) : Ptr{Float64}(C_NULL))::Ptr{Float64}, dopt::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return (dR, dmu, dalpha, dtheta, dsig, dopt, info)
end

"""
    lg_set_tip_noise!(obj, families, sigma_e; scale = ones(length(families)), se2 = nothing)

Measurement error at the tips (pgbp_lg_set_tip_noise): the conditional variance of every listed tip family (0-based indices
into the family table given to pgbp_lg_setup) gains `scale[f] * sigma_e + Diagonal(se2[:, f])`.  `sigma_e` is `p x p`
symmetric, or `p x p x n_sites` for one per site (`se2` is then `p x length(families) x n_sites`); `se2` may be `nothing`.
An empty `families` clears the noise; the call replaces the previous list.  The next pgbp_lg_assignfactors or
pgbp_enqueue_loglik_lg uses it; the sweeps read the current noise (lg_loo and lg_impute then predict the observation of a
noisy tip).  An invalid entry is an error and nothing changes.
"""
function lg_set_tip_noise!(o::DeviceClusterGraphBelief, families::AbstractVector{<:Integer}, sigma_e::AbstractArray{Float64};
                           scale::AbstractVector{<:Real} = ones(Base.length(families)),
                           se2::Union{Nothing,AbstractArray{Float64}} = nothing)
    fam = Vector{Int32}(families)
    sc = Vector{Float64}(scale)
    sig = Array{Float64}(sigma_e)
    per_site = ndims(sig) == 3 ? Int32(1) : Int32(0)
    s2 = se2 === nothing ? Ptr{Float64}(C_NULL) : Array{Float64}(se2)
    check(o.handle, @ccall LIB.pgbp_lg_set_tip_noise(o.handle::Ptr{Cvoid}, Int32(Base.length(fam))::Int32, fam::Ptr{Int32},
                                                     sc::Ptr{Float64}, sig::Ptr{Float64}, s2::Ptr{Float64},
                                                     per_site::Int32)::Cint)
    return nothing
end

"""
    lg_tip_noise_count(obj) -> Int

Number of noisy tips in force (pgbp_lg_tip_noise_count): 0 when none is set, -1 without a family table.
"""
lg_tip_noise_count(o::DeviceClusterGraphBelief) = Int(@ccall LIB.pgbp_lg_tip_noise_count(o.handle::Ptr{Cvoid})::Int32)

"""
    lg_set_site_missing!(obj, missing)

Per-site missing tips of a univariate batch (pgbp_lg_set_site_missing): `missing` is an `n_rows x n_sites` array of Bool (or
any integer type), `true` where the tip with that data row is NOT observed at that site; `nothing` clears the mask.  Accepted
only on a thread-per-site engine (p = 1, every belief of at most 2 variables, at least 8 sites).  The call replaces the previous
mask; the next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg uses it, and the lanes-are-sites sweeps read it.  A row without
a tip, a tip the set-up's child_mask already skips, or a site left with nothing observed is an error and nothing changes.
"""
function lg_set_site_missing!(o::DeviceClusterGraphBelief, missing::Union{Nothing,AbstractMatrix})
    m = missing === nothing ? Ptr{UInt8}(C_NULL) : Matrix{UInt8}(missing .!= 0)
    check(o.handle, @ccall LIB.pgbp_lg_set_site_missing(o.handle::Ptr{Cvoid}, m::Ptr{UInt8})::Cint)
    return nothing
end

"""
    lg_site_missing(obj, n_rows, n_sites) -> Matrix{Bool}

The mask in force (pgbp_lg_get_site_missing), `n_rows x n_sites`; all `false` when none is set.
"""
function lg_site_missing(o::DeviceClusterGraphBelief, n_rows::Integer, n_sites::Integer)
    m = zeros(UInt8, max(n_rows, 1), max(n_sites, 1))
    check(o.handle, @ccall LIB.pgbp_lg_get_site_missing(o.handle::Ptr{Cvoid}, m::Ptr{UInt8})::Cint)
    return reshape(m[1:n_rows * n_sites], n_rows, n_sites) .!= 0
end

"""
    lg_site_missing_count(obj) -> Int

Number of masked (row, site) pairs in force (pgbp_lg_site_missing_count): 0 when no mask is set, -1 without a family table.
"""
lg_site_missing_count(o::DeviceClusterGraphBelief) = Int(@ccall LIB.pgbp_lg_site_missing_count(o.handle::Ptr{Cvoid})::Int32)

"""
    lg_shift_scan(obj, p, nfamilies; min_info = 1e-8) -> (jump, lr, identified, information)

Every edge scanned for a mean shift from the current beliefs (pgbp_lg_shift_scan: one sweep over the node families).  Per
family f of the table given to pgbp_lg_setup: `jump[:, f]` the maximum-likelihood displacement of the child's conditional mean
(NaN at a trait outside the family's child_mask or not identified, and for a root-prior family), `lr[f]` the gain
2 (ll(jump) - ll(0)), `identified[f]` the bit mask of kept traits and `information[:, :, f]` the observed information H_f at the
kept traits (NaN elsewhere).  The shift on parent edge k is `jump / gamma_k`, its information `gamma_k^2 H_f`.  A trait whose
pivot in H_f is not above `min_info` times its prior precision is not identified and is dropped.  With shifts set the result is
the increment to an edge's shift, the others held.  Exact under the condition of `lg_gradient`.  A cluster that is not
positive definite throws its PosDefException.
"""
function lg_shift_scan(o::DeviceClusterGraphBelief, p::Integer, nfamilies::Integer; min_info::Real = 1e-8)
    n = max(nfamilies, 1)
    jump = zeros(p, n); lr = zeros(n); identified = zeros(UInt64, n); information = zeros(p, p, n)
    info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_lg_shift_scan(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32, Float64(min_info)::Float64, jump::Ptr{Float64}, lr::Ptr{Float64}, identified::Ptr{UInt64}, information::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (jump[:, 1:nfamilies], lr[1:nfamilies], identified[1:nfamilies], information[:, :, 1:nfamilies])
end

"""
    sample_size(obj) -> Int

Doubles per draw of `sample_posterior!`: the sum of the cluster dimensions (pgbp_sample_size).
"""
sample_size(o::DeviceClusterGraphBelief) = Int(@ccall LIB.pgbp_sample_size(o.handle::Ptr{Cvoid})::Int64)

"""
    sample_posterior!(obj, ndraws = 1; z = randn(sample_size(obj), ndraws), tree = 1) -> x

Joint posterior draws of every cluster variable from the current beliefs (pgbp_sample_posterior): one preorder sweep of schedule
tree `tree` (1-based, into the schedule given to `set_schedule!`) that conditions each cluster on the sepset to its parent.
Column d of `x` is draw d: cluster i's variables at the cumulative offset of the cluster dimensions, in the belief's own order;
`z = 0` gives the joint posterior mean.  A draw from the joint posterior only when the beliefs are calibrated (postorder and
preorder) on a clique tree; the call does not verify that.  A cluster whose conditional precision is not positive definite
throws its PosDefException (info = the cluster's index).
"""
function sample_posterior!(o::DeviceClusterGraphBelief, ndraws::Integer = 1;
                           z::AbstractMatrix{Float64} = randn(sample_size(o), ndraws), tree::Integer = 1)
    size(z) == (sample_size(o), ndraws) || error("z must be sample_size(obj) x ndraws")
    zz = Matrix{Float64}(z); x = zeros(max(sample_size(o), 1), ndraws); info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_sample_posterior(o.handle::Ptr{Cvoid}, (tree-1)::Int32, Int32(0)::Int32, Int32(1)::Int32, ndraws::Int32, zz::Ptr{Float64}, x::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return x[1:sample_size(o), :]
end

"""
    posterior_cov(obj, c; tree = 1) -> (w, k)

Exact posterior covariances of linear functionals of the cluster variables (pgbp_posterior_cov): the adjoint of
`sample_posterior!`'s sweep `x = m + A z`.  `c` is `sample_size(obj) x ncols`, a weight per entry of a draw; column `a` of `w` is
`A'c_a` (`w[:, a]' * w[:, b]` is the posterior covariance of the functionals `a` and `b`), column `a` of `k` is `A w_a`, the
covariance of every entry with functional `a`.  Exact only when the beliefs are calibrated on a clique tree; the call does not
verify that.  A cluster whose conditional precision is not positive definite throws its PosDefException.
"""
function posterior_cov(o::DeviceClusterGraphBelief, c::AbstractVecOrMat{Float64}; tree::Integer = 1)
    cc = Matrix{Float64}(reshape(c, size(c, 1), :)); ncols = size(cc, 2)
    size(cc, 1) == sample_size(o) || error("c must be sample_size(obj) x ncols")
    w = zeros(max(sample_size(o), 1), ncols); k = zeros(max(sample_size(o), 1), ncols); info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_posterior_cov(o.handle::Ptr{Cvoid}, (tree-1)::Int32, Int32(0)::Int32, Int32(1)::Int32, ncols::Int32, cc::Ptr{Float64}, w::Ptr{Float64}, k::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (w[1:sample_size(o), :], k[1:sample_size(o), :])
end

# ---- the model run forwards (pgbp_lg_set_topology, pgbp_lg_set_data / pgbp_lg_get_data, pgbp_lg_simulate).  Like the rest
# of this file these wrappers are NOT exercised in the build container (no Julia there); tests/test_gpu_simulate.py drives the
# same five C functions through the ctypes mirror.

"""
    lg_set_topology!(obj, parent_family)

Node topology of the family table (pgbp_lg_set_topology): `parent_family` is `max_parents x n_families`, entry `(k, f)` the
0-based family whose child is parent `k` of family `f`; -1: the fixed root; -2: a root without a proper prior (`lg_simulate`
is then refused).  Parents come before their children.  An invalid entry is an error that names it, and nothing changes.
"""
function lg_set_topology!(o::DeviceClusterGraphBelief, parent_family::AbstractArray{<:Integer})
    pf = Array{Int32}(parent_family)
    check(o.handle, @ccall LIB.pgbp_lg_set_topology(o.handle::Ptr{Cvoid}, pf::Ptr{Int32})::Cint)
    return nothing
end

"""
    lg_set_data!(obj, data; sites = nothing)

Replace the tip data given to pgbp_lg_setup without a new set-up (pgbp_lg_set_data): `data` is `p x n_rows x length(sites)`,
`sites` a 1-based unit range (default: as many sites as `data` has, from the first).  The missing-data pattern stays the
set-up's.  The next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg uses the new data; nothing is refilled by this call.
"""
function lg_set_data!(o::DeviceClusterGraphBelief, data::AbstractArray{Float64}; sites::Union{Nothing,UnitRange{Int}} = nothing)
    d = Array{Float64}(data)
    r = sites === nothing ? (1:size(d, 3)) : sites
    check(o.handle, @ccall LIB.pgbp_lg_set_data(o.handle::Ptr{Cvoid}, Int32(first(r) - 1)::Int32, Int32(last(r))::Int32,
                                                d::Ptr{Float64})::Cint)
    return nothing
end

"""
    lg_get_data(obj, p, nrows, sites) -> data

The tip data the device holds for the 1-based unit range `sites` (pgbp_lg_get_data): `p x nrows x length(sites)`.
"""
function lg_get_data(o::DeviceClusterGraphBelief, p::Integer, nrows::Integer, sites::UnitRange{Int})
    d = zeros(p, nrows, Base.length(sites))
    check(o.handle, @ccall LIB.pgbp_lg_get_data(o.handle::Ptr{Cvoid}, Int32(first(sites) - 1)::Int32, Int32(last(sites))::Int32,
                                                d::Ptr{Float64})::Cint)
    return d
end

"""
    lg_simulate(obj, p, nfamilies, sites; z = nothing, seed = 0, write_data = false) -> (x, info)

Every node of the network drawn from the current model (pgbp_lg_simulate) for the 1-based unit range `sites` (replicates):
`x` is `p x nfamilies x length(sites)`, family order; `info[s]` is 0, or the 1-based family whose conditional variance is not
positive definite (that site's `x` is NaN).  `z` (same shape as `x`) are the caller's standard normals -- `z = 0` gives the
prior means --; with `z = nothing` the device draws them from `seed` (Philox4x32-10 and Box-Muller: include/pgbp.h has the
recipe).  `write_data = true` puts the tips' observed traits into the engine's data, as `lg_set_data!` would.
"""
function lg_simulate(o::DeviceClusterGraphBelief, p::Integer, nfamilies::Integer, sites::UnitRange{Int};
                     z::Union{Nothing,AbstractArray{Float64}} = nothing, seed::Integer = 0, write_data::Bool = false)
    n = Base.length(sites)
    x = zeros(p, nfamilies, n); info = zeros(Int32, n)
    zz = z === nothing ? Ptr{Float64}(C_NULL) : Array{Float64}(z)
    z === nothing || size(zz) == size(x) || error("z must be p x nfamilies x length(sites)")
    check(o.handle, @ccall LIB.pgbp_lg_simulate(o.handle::Ptr{Cvoid}, Int32(first(sites) - 1)::Int32, Int32(last(sites))::Int32,
                                                zz::Ptr{Float64}, UInt64(seed)::UInt64, x::Ptr{Float64},
                                                Ptr{Float64}(C_NULL)::Ptr{Float64}, Int32(write_data)::Int32,
                                                info::Ptr{Int32})::Cint)
    return x, info
end

"""
    simulate_scratch_limits(factor_doubles, state_doubles)

Process-wide bounds of the scratch of `lg_simulate` in doubles (pgbp_simulate_scratch_limits); a value <= 0 restores the default.
"""
simulate_scratch_limits(factor_doubles::Integer, state_doubles::Integer) =
    @ccall LIB.pgbp_simulate_scratch_limits(Int64(factor_doubles)::Int64, Int64(state_doubles)::Int64)::Cvoid

"the reference's error line for a failed message (src/beliefupdates.jl:69-76): belief metadata + integrated indices"
function report_failure(o::DeviceClusterGraphBelief, spt, res::Result, verbose::Bool)
    i = res.fail_edge + 1
    sender = res.fail_dir == 0 ? spt[4][i] : spt[3][i]
    sep = o.cgb.belief[PGBP.sepsetindex(spt[1][i], spt[2][i], o.cgb)]
    integ = setdiff(1:length(o.cgb.belief[sender].h), PGBP.scopeindex(sep, o.cgb.belief[sender]))
    verbose && @error "belief $(o.cgb.belief[sender].metadata), integrating $(integ)"
    return PGBP.BPPosDefException("belief $(o.cgb.belief[sender].metadata), integrating $(integ)", res.fail_info)
end

"""
    propagate_belief!(o, to, sepset, from; update_residualnorm = true) -> nothing | BPPosDefException

`propagate_belief!(cluster_to, sepset, cluster_from, residual)` (src/beliefupdates.jl:634-649) by belief index (1-based,
sepset index >= nclusters + 1): the exception is RETURNED, not thrown, and nothing of the message is applied.
"""
function PGBP.propagate_belief!(o::DeviceClusterGraphBelief, to::Integer, sepset::Integer, from::Integer;
                                update_residualnorm::Bool=true)
    info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_propagate(o.handle::Ptr{Cvoid}, (to-1)::Int32, (sepset-1)::Int32, (from-1)::Int32,
        Ref(Opts(0, update_residualnorm, 0, 0, 1e-5))::Ref{Opts}, info::Ref{Int32})::Cint)
    pull!(o)
    info[] == 0 && return nothing
    sep = o.cgb.belief[sepset]
    integ = setdiff(1:length(o.cgb.belief[from].h), PGBP.scopeindex(sep, o.cgb.belief[from]))
    return PGBP.BPPosDefException("belief $(o.cgb.belief[from].metadata), integrating $(integ)", info[])
end

function traverse!(o::DeviceClusterGraphBelief, spt, dir::Integer, verbose, up_rn, up_kl)
    set_schedule!(o, [spt])
    r = Ref(Result(0,0,0,0,0,0,0,0,0,0))
    check(o.handle, @ccall LIB.pgbp_traverse(o.handle::Ptr{Cvoid}, 0::Int32, dir::Int32,
        Ref(Opts(0, up_rn, up_kl, 0, 1e-5))::Ref{Opts}, r::Ref{Result})::Cint)
    pull!(o)
    r[].succ != 0 && return true
    report_failure(o, spt, r[], verbose)
    return false
end
"propagate_1traversal_postorder!(beliefs, pa_lab, ch_lab, pa_j, ch_j, verbose, up_rn, up_kl) -> Bool (src/calibration.jl:111-135)"
PGBP.propagate_1traversal_postorder!(o::DeviceClusterGraphBelief, pa_lab, ch_lab, pa_j, ch_j,
        verbose::Bool=true, up_rn::Bool=true, up_kl::Bool=false) =
    traverse!(o, (pa_lab, ch_lab, pa_j, ch_j), 0, verbose, up_rn, up_kl)
"propagate_1traversal_preorder! (src/calibration.jl:137-161)"
PGBP.propagate_1traversal_preorder!(o::DeviceClusterGraphBelief, pa_lab, ch_lab, pa_j, ch_j,
        verbose::Bool=true, up_rn::Bool=true, up_kl::Bool=false) =
    traverse!(o, (pa_lab, ch_lab, pa_j, ch_j), 1, verbose, up_rn, up_kl)

"regularizebeliefs_bycluster!(beliefs, clustergraph) (src/clustergraphbeliefs.jl:235-275) on the device (the graph is the engine's)"
function PGBP.regularizebeliefs_bycluster!(o::DeviceClusterGraphBelief, _clustergraph=nothing)
    check(o.handle, @ccall LIB.pgbp_regularize_bycluster(o.handle::Ptr{Cvoid})::Cint)
    pull!(o)
end

"""
    regularizebeliefs_onschedule!(beliefs, clustergraph)

src/clustergraphbeliefs.jl:343-403 on the device (the graph is the engine's): the walk levelled once per graph, a few
launches per level, bit for bit the sequential walk.  Throws the BPPosDefException of the first failing message in walk
order, as the reference does.
"""
function PGBP.regularizebeliefs_onschedule!(o::DeviceClusterGraphBelief, _cg=nothing)
    fail_msg = Ref(Int32(-1)); fail_info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_regularize_onschedule(o.handle::Ptr{Cvoid}, Int32(0)::Int32, Int32(1)::Int32,
        Ref(Opts(0, 1, 0, 0, 1e-5))::Ref{Opts}, fail_msg::Ref{Int32}, fail_info::Ref{Int32})::Cint)
    pull!(o)
    fail_msg[] < 0 && return nothing
    j = o.cgb.nclusters + fail_msg[] ÷ 2 + 1                # message 2(k-1) + dir - 1 is received by the sepset's end `dir`
    lab = o.cgb.belief[j].metadata[fail_msg[] % 2 == 0 ? 2 : 1]
    from = PGBP.clusterindex(lab, o.cgb)
    integ = setdiff(1:length(o.cgb.belief[from].h), PGBP.scopeindex(o.cgb.belief[j], o.cgb.belief[from]))
    throw(PGBP.BPPosDefException("belief $(o.cgb.belief[from].metadata), integrating $(integ)", fail_info[]))
end

"free_energy(beliefs) -> (average energy, approximate entropy, free energy) (src/score.jl:162-182)"
function PGBP.free_energy(o::DeviceClusterGraphBelief)
    out = zeros(3); info = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_free_energy(o.handle::Ptr{Cvoid}, out::Ptr{Float64}, info::Ref{Int32})::Cint)
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return (out[1], out[2], out[3])
end
"factored_energy(beliefs) (src/score.jl:151-154)"
PGBP.factored_energy(o::DeviceClusterGraphBelief) = (f = PGBP.free_energy(o); (f[1], f[2], -f[3]))

"""
    residual_kldiv!(o, to, sepset, from) -> iscalibrated_kl

`residual_kldiv!(messageresidual[(to, from)], sepset)` (src/beliefs.jl:1060-1075) for the message last sent from `from`
to `to`; the residual's `kldiv` / `iscalibrated_kl` are updated in the Julia object by the pull.
"""
function PGBP.residual_kldiv!(o::DeviceClusterGraphBelief, to::Integer, sepset::Integer, from::Integer)
    flag = Ref(Int32(0))
    check(o.handle, @ccall LIB.pgbp_residual_kldiv(o.handle::Ptr{Cvoid}, (to-1)::Int32, (sepset-1)::Int32, (from-1)::Int32,
        Ref(Opts(0, 1, 1, 0, 1e-5))::Ref{Opts}, flag::Ref{Int32})::Cint)
    pull!(o)
    return flag[] != 0
end

"init_beliefs_reset_fromfactors! (src/clustergraphbeliefs.jl:126-139) / init_messagecalibrationflags_reset! (:146-150)"
function PGBP.init_beliefs_reset_fromfactors!(o::DeviceClusterGraphBelief)
    check(o.handle, @ccall LIB.pgbp_reset_from_factors(o.handle::Ptr{Cvoid})::Cint); pull!(o)
end
function PGBP.init_messagecalibrationflags_reset!(o::DeviceClusterGraphBelief, reset_kl::Bool=true)
    check(o.handle, @ccall LIB.pgbp_reset_flags(o.handle::Ptr{Cvoid}, reset_kl::Int32)::Cint); pull!(o)
end

# ---- factor assignment on the device (include/pgbp.h: pgbp_lg_families / pgbp_lg_params) --------------------------
struct LgFamilies      # pgbp_lg_families
    p::Int32; n_families::Int32; max_parents::Int32; n_rates::Int32; n_rows::Int32
    cluster::Ptr{Int32}; n_parents::Ptr{Int32}; child_pos::Ptr{Int32}; data_row::Ptr{Int32}
    parent_pos::Ptr{Int32}; length::Ptr{Float64}; gamma::Ptr{Float64}; color::Ptr{Int32}; data::Ptr{Float64}
    child_mask::Ptr{UInt64}; parent_mask::Ptr{UInt64}     # C_NULL: complete data
end
struct LgParams        # pgbp_lg_params
    model::Int32; per_site::Int32; R::Ptr{Float64}; alpha::Ptr{Float64}; theta::Ptr{Float64}; mu::Ptr{Float64}
end

"""
    lg_setup!(o, prenodes, tbl, taxa, colorof = e -> 0; nrates = 1, rootpriorcolor = nothing)

Static part of `assignfactors!` (src/beliefs.jl:786-861): one entry per node family that carries a factor, in the order of
its loop over `node2cluster`; `colorof(edge)` is the 0-based index of the parent edge's variance rate
(`HeterogeneousBrownianMotion`: its colour; homogeneous models: 0).  A RANDOM root with a PROPER prior (`factor_root`,
src/evomodels/evomodels.jl:377-396) needs `rootpriorcolor` = the 0-based index, among the `rates` later given to
`loglik!`, of the prior variance (append it to the model's rates and count it in `nrates`); a fixed root or an improper
prior has no factor and takes `nothing` -- asking for a factor the model does not have, or omitting one it has, is an
error here rather than a silently different likelihood.  Missing tip values (`missing` in `tbl`) and partial scopes are
passed as scope masks (bit t = trait t), as `pgbp_amd/factors.py` does.  Call once per cluster graph.
"""
function lg_setup!(o::DeviceClusterGraphBelief, prenodes, tbl, taxa, colorof = e -> 0; nrates::Integer = 1,
                   rootpriorcolor::Union{Nothing,Integer} = nothing)
    cgb = o.cgb; b = cgb.belief; p = length(tbl)
    p <= 64 || error("at most 64 traits")
    n2c, n2fam, n2fix = cgb.node2cluster, cgb.node2family, cgb.node2fixed
    K = max(1, maximum(length(nf) - 1 for nf in n2fam))
    cl = Int32[]; np = Int32[]; cpos = Int32[]; drow = Int32[]
    ppos = Int32[]; len = Float64[]; gam = Float64[]; col = Int32[]
    cmask = UInt64[]; pmask = UInt64[]
    full = p == 64 ? typemax(UInt64) : (UInt64(1) << p) - UInt64(1)
    partial = false
    # (first variable of the node's block or -1, mask of its traits in scope) inside cluster belief `be`
    function place(be, lab)
        j = findfirst(isequal(lab), PGBP.nodelabels(be))
        insc = PGBP.inscope(be)                                   # p x k BitArray (src/beliefs.jl:72-100)
        nd = [count(insc[:, c]) for c in 1:size(insc, 2)]
        any(x -> x != 0 && x != p, nd) && (partial = true)
        m = reduce(|, (UInt64(1) << (t - 1) for t in 1:p if insc[t, j]); init = UInt64(0))
        return (nd[j] == 0 ? Int32(-1) : Int32(sum(nd[1:j-1])), m)
    end
    observed(row) = (ok = [!ismissing(tbl[v][row]) for v in 1:p]; all(ok) || (partial = true);
                     reduce(|, (UInt64(1) << (t - 1) for t in 1:p if ok[t]); init = UInt64(0)))
    for (ni, ci) in enumerate(n2c)
        nf = n2fam[ni]; be = b[ci]; ch = prenodes[ni]
        if length(nf) == 1                                        # the root's own family: its prior, if it has one
            ni == 1 || error("only the root node can belong to a family of size 1")
            if n2fix[1]
                rootpriorcolor === nothing || error("the root is fixed: it has no prior factor")
                continue
            end
            rootpriorcolor === nothing && continue                # improper prior: no factor (evomodels.jl:383-385)
            (pos, m) = place(be, nf[1])
            push!(cl, ci - 1); push!(np, 0); push!(cpos, pos); push!(drow, -1); push!(cmask, m)
            for k in 1:K
                push!(ppos, -1); push!(len, 1.0); push!(gam, 1.0); push!(col, k == 1 ? Int32(rootpriorcolor) : Int32(0))
                push!(pmask, full)
            end
            continue
        end
        push!(cl, ci - 1); push!(np, length(nf) - 1)
        if n2fix[ni]                                              # a tip: its data row is absorbed
            row = findfirst(isequal(ch.name), taxa)
            push!(cpos, -1); push!(drow, Int32(row - 1)); push!(cmask, observed(row))
        else
            (pos, m) = place(be, nf[1])
            push!(cpos, pos); push!(drow, -1); push!(cmask, m)
        end
        for k in 1:K
            if k < length(nf)
                pa = prenodes[nf[k+1]]
                e = first(e for e in pa.edge if PGBP.getchild(e) === ch)            # src/beliefs.jl:813-820
                if n2fix[nf[k+1]]
                    push!(ppos, -1); push!(pmask, full)
                else
                    (pos, m) = place(be, nf[k+1]); push!(ppos, pos); push!(pmask, m)
                end
                push!(len, e.length); push!(gam, length(nf) > 2 ? e.gamma : 1.0); push!(col, colorof(e))
            else
                push!(ppos, -1); push!(len, 1.0); push!(gam, 1.0); push!(col, 0); push!(pmask, full)
            end
        end
    end
    data = Float64[ismissing(tbl[v][r]) ? NaN : tbl[v][r] for v in 1:p, r in 1:length(taxa)]   # [row][trait], row-major for C
    o.keep = (cl, np, cpos, drow, ppos, len, gam, col, data, cmask, pmask)            # keep alive
    f = LgFamilies(p, length(cl), K, nrates, length(taxa), pointer(cl), pointer(np), pointer(cpos), pointer(drow),
                   pointer(ppos), pointer(len), pointer(gam), pointer(col), pointer(data),
                   partial ? pointer(cmask) : C_NULL, partial ? pointer(pmask) : C_NULL)
    GC.@preserve cl np cpos drow ppos len gam col data cmask pmask check(o.handle,
        @ccall LIB.pgbp_lg_setup(o.handle::Ptr{Cvoid}, Ref(f)::Ref{LgFamilies})::Cint)
end

"""
    loglik!(o, rates, mu; alpha = nothing, theta = nothing)

The body of `score(θ)` (src/calibration.jl:195-221) on the device: factors from the model parameters, postorder of
schedule tree 1, `integratebelief!` at its root cluster.  `rates`: vector of p×p variance matrices
(OU: the stationary variance).  Only the parameters and the result cross the bus.
"""
function loglik!(o::DeviceClusterGraphBelief, rates::Vector{<:AbstractMatrix}, mu::AbstractVector;
                 alpha = nothing, theta = nothing)
    R = Float64.(reduce(vcat, vec.(rates))); m = Float64.(mu)
    ou = alpha !== nothing
    a = ou ? Float64[alpha] : Float64[0]; th = ou ? Float64.(theta) : zeros(length(m))
    prm = LgParams(ou ? 1 : 0, 0, pointer(R), ou ? pointer(a) : C_NULL, ou ? pointer(th) : C_NULL, pointer(m))
    norm = Ref(0.0); info = Ref(Int32(0))
    GC.@preserve R m a th begin
        check(o.handle, @ccall LIB.pgbp_lg_assignfactors(o.handle::Ptr{Cvoid}, Ref(prm)::Ref{LgParams})::Cint)
        check(o.handle, @ccall LIB.pgbp_enqueue_loglik_lg(o.handle::Ptr{Cvoid}, 1::Int32, Ref(Opts(0, 1, 0, 0, 1e-5))::Ref{Opts})::Cint)
        check(o.handle, @ccall LIB.pgbp_fetch_loglik(o.handle::Ptr{Cvoid}, norm::Ref{Float64}, info::Ref{Int32})::Cint)
    end
    info[] == 0 || throw(PGBP.LA.PosDefException(info[]))
    return norm[]
end

# ---- several GPUs (include/pgbp.h "several GPUs") -----------------------------------------------------------------
# One process, several devices: a group of engines over contiguous site ranges; every call fans out inside libpgbp.so.
mutable struct DeviceGroup
    handle::Ptr{Cvoid}
    n_sites::Int
    packed_size::Int
end
checkg(g, rc) = rc == 0 || error(unsafe_string(@ccall LIB.pgbp_group_last_error(g::Ptr{Cvoid})::Cstring))

"`n_sites` independent replicas (same graph and scopes as `o`, different numbers) sharded over `devices` (0-based ordinals)"
function DeviceGroup(dims::Vector{Int32}, sepcl::Vector{Int32}, off::Vector{Int64}, idx::Vector{Int32},
                     nclusters::Integer, n_sites::Integer, devices::Vector{Int32})
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve dims sepcl off idx devices begin
        d = Desc(nclusters, length(dims) - nclusters, pointer(dims), pointer(sepcl), pointer(off), pointer(idx), n_sites, 0)
        rc = @ccall LIB.pgbp_group_create(Ref(d)::Ref{Desc}, length(devices)::Int32, devices::Ptr{Int32}, h::Ref{Ptr{Cvoid}})::Cint
        rc == 0 || error(unsafe_string(@ccall LIB.pgbp_group_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    end
    g = DeviceGroup(h[], n_sites, sum(m*m + m + 1 for m in Int.(dims)))
    finalizer(x -> @ccall(LIB.pgbp_group_destroy(x.handle::Ptr{Cvoid})::Cvoid), g)
    return g
end
"packed: [packed_size, n_sites] (one column per site)"
set_beliefs!(g::DeviceGroup, packed::Matrix{Float64}) =
    checkg(g.handle, @ccall LIB.pgbp_group_set_beliefs(g.handle::Ptr{Cvoid}, packed::Ptr{Float64}, 1::Int32)::Cint)
function set_schedule!(g::DeviceGroup, schedule)
    off = Int32[0]; pa = Int32[]; ch = Int32[]
    for spt in schedule
        append!(pa, Int32.(spt[3] .- 1)); append!(ch, Int32.(spt[4] .- 1)); push!(off, length(pa))
    end
    checkg(g.handle, @ccall LIB.pgbp_group_set_schedule(g.handle::Ptr{Cvoid}, length(schedule)::Int32, off::Ptr{Int32}, pa::Ptr{Int32}, ch::Ptr{Int32})::Cint)
end
"calibrate! on every site -> vector of (succ, iscal), one per site"
function PGBP.calibrate!(g::DeviceGroup, niter::Integer=1; auto::Bool=false, update_residualnorm::Bool=true)
    res = Vector{Result}(undef, g.n_sites)
    checkg(g.handle, @ccall LIB.pgbp_group_calibrate(g.handle::Ptr{Cvoid}, niter::Int32,
        Ref(Opts(auto, update_residualnorm, 0, 0, 1e-5))::Ref{Opts}, res::Ptr{Result})::Cint)
    return [(r.succ != 0, r.iscal != 0) for r in res]
end
"per-site integratebelief! norms (the log-likelihoods on a calibrated clique tree)"
function loglik(g::DeviceGroup, j::Integer)
    norm = zeros(g.n_sites); info = zeros(Int32, g.n_sites)
    checkg(g.handle, @ccall LIB.pgbp_group_integrate(g.handle::Ptr{Cvoid}, (j-1)::Int32, C_NULL::Ptr{Float64}, norm::Ptr{Float64}, info::Ptr{Int32})::Cint)
    any(!=(0), info) && throw(PGBP.LA.PosDefException(first(filter(!=(0), info))))
    return norm
end

# Sites with different missing-data patterns behind one handle: one pgbp_desc per pattern (its own scopes), `sites` = for
# every pattern in turn the (1-based) global indices of its sites.  Pattern k's engine takes everything pattern-specific.
mutable struct DevicePatterns
    handle::Ptr{Cvoid}
    n_sites::Int
end
function DevicePatterns(descs::Vector{Desc}, sites::Vector{<:Integer})
    refs = [Ref(d) for d in descs]
    ptrs = [Base.unsafe_convert(Ptr{Desc}, r) for r in refs]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    s0 = Int32.(sites .- 1)
    rc = GC.@preserve refs @ccall LIB.pgbp_patterns_create(Int32(length(descs))::Int32, ptrs::Ptr{Ptr{Desc}}, s0::Ptr{Int32},
                                                         h::Ref{Ptr{Cvoid}})::Cint
    rc == 0 || error(unsafe_string(@ccall LIB.pgbp_patterns_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    g = DevicePatterns(h[], length(sites))
    finalizer(x -> @ccall(LIB.pgbp_patterns_destroy(x.handle::Ptr{Cvoid})::Cvoid), g)
    return g
end
checkp(h, rc) = rc == 0 || error(unsafe_string(@ccall LIB.pgbp_patterns_last_error(h::Ptr{Cvoid})::Cstring))
pattern_engine(g::DevicePatterns, k::Integer) = @ccall LIB.pgbp_patterns_engine(g.handle::Ptr{Cvoid}, Int32(k - 1)::Int32)::Ptr{Cvoid}
function set_schedule!(g::DevicePatterns, off::Vector{Int32}, pa::Vector{Int32}, ch::Vector{Int32})
    checkp(g.handle, @ccall LIB.pgbp_patterns_set_schedule(g.handle::Ptr{Cvoid}, Int32(length(off) - 1)::Int32, off::Ptr{Int32},
                                                           pa::Ptr{Int32}, ch::Ptr{Int32})::Cint)
end
function PGBP.calibrate!(g::DevicePatterns, niter::Integer=1; auto=false, update_residualnorm=true)
    res = Vector{Result}(undef, g.n_sites)
    checkp(g.handle, @ccall LIB.pgbp_patterns_calibrate(g.handle::Ptr{Cvoid}, Int32(niter)::Int32,
        Ref(Opts(auto, update_residualnorm, 0, 0, 1e-5))::Ref{Opts}, res::Ptr{Result})::Cint)
    return [(r.succ != 0, r.iscal != 0) for r in res]
end
"score() body of every site (device factor fill + postorder + root integrate), in the caller's site order"
function loglik_lg(g::DevicePatterns)
    checkp(g.handle, @ccall LIB.pgbp_patterns_enqueue_loglik_lg(g.handle::Ptr{Cvoid}, Int32(1)::Int32,
        Ref(Opts(0, 1, 0, 0, 1e-5))::Ref{Opts})::Cint)
    norm = zeros(g.n_sites); info = zeros(Int32, g.n_sites)
    checkp(g.handle, @ccall LIB.pgbp_patterns_fetch_loglik(g.handle::Ptr{Cvoid}, norm::Ptr{Float64}, info::Ptr{Int32})::Cint)
    return norm, info
end

# One process per GPU (Distributed.jl / MPI.jl workers): ONE ncclAllGather per gather.
const COMM_ID_BYTES = 128
"rank 0: the id to hand to the other ranks (e.g. `MPI.bcast`, `remotecall_fetch`)"
function comm_unique_id()
    id = zeros(UInt8, COMM_ID_BYTES)
    rc = @ccall LIB.pgbp_comm_unique_id(id::Ptr{UInt8})::Cint
    rc == 0 || error(unsafe_string(@ccall LIB.pgbp_comm_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    return id
end
"0 if this rank can open its communicator (RCCL loadable, the device exists): agree on the minimum over the ranks
BEFORE the collective `comm_create` -- a rank that failed there alone would leave its peers inside ncclCommInitRank"
comm_precheck(device::Integer) = @ccall LIB.pgbp_comm_precheck(device::Int32)::Cint
function comm_create(id::Vector{UInt8}, n_ranks::Integer, rank::Integer, device::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.pgbp_comm_create(id::Ptr{UInt8}, n_ranks::Int32, rank::Int32, device::Int32, h::Ref{Ptr{Cvoid}})::Cint
    rc == 0 || error(unsafe_string(@ccall LIB.pgbp_comm_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    return h[]
end
"every rank's per-site log-likelihoods on every rank + min over all sites of (succ, iscal): one collective"
function comm_gather_loglik(comm::Ptr{Cvoid}, o::DeviceClusterGraphBelief, n_ranks::Integer, slot_sites::Integer)
    norm = zeros(slot_sites, n_ranks); info = zeros(Int32, slot_sites, n_ranks); succ = Ref(Int32(0)); iscal = Ref(Int32(0))
    rc = @ccall LIB.pgbp_comm_gather_loglik(comm::Ptr{Cvoid}, o.handle::Ptr{Cvoid}, slot_sites::Int32, norm::Ptr{Float64},
                                            info::Ptr{Int32}, succ::Ref{Int32}, iscal::Ref{Int32})::Cint
    rc == 0 || error(unsafe_string(@ccall LIB.pgbp_comm_last_error(comm::Ptr{Cvoid})::Cstring))
    return (norm, info, succ[] != 0, iscal[] != 0)
end

end # module
