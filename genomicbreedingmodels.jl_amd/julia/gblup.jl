# gblup.jl — the reference-side binding a GenomicBreedingModels.jl maintainer adds to call
# libgbm.so (MI355X GRM + GBLUP core). Drop into src/ next to linear.jl, `include("gblup.jl")`
# after linear.jl (src/GenomicBreedingModels.jl:25-33), export `gblup` next to `ridge`
# (src/GenomicBreedingModels.jl:46) and add "gblup" to `linear_models` in predict
# (src/prediction.jl:225). Julia is not available in the build container, so this file is not
# executed by the test suite; the Python mirror (gbm/linear.py) exercises the same C ABI with
# the same argument layout (column-major Float64, Int64 dimensions).

const LIBGBM = get(ENV, "GBM_LIBRARY", joinpath(@__DIR__, "..", "gbm", "libgbm.so"))

function gbm_last_error()::String
    unsafe_string(ccall((:gbm_last_error, LIBGBM), Cstring, ()))
end

# GRM arithmetic (include/gbm.h GBM_GRM_*): :auto = exact int8-MFMA GRM when the allele frequencies are
# diploid dosages/2 (2x ∈ {0, 1, 2} in every cell, checked on the device), else the fp64-MFMA SYRK
# :dropin (gblup's default) = the GBM_GRM variable when it is set, else :auto
const GBM_GRM_MODES = Dict(:default => Cint(-1), :fp64 => Cint(0), :exact => Cint(1), :auto => Cint(2),
                           :dropin => Cint(3))

function gbm_grm_mode(grm::Symbol)::Cint
    haskey(GBM_GRM_MODES, grm) || throw(ArgumentError("grm must be :dropin, :auto, :exact, :fp64 or :default, got :$grm"))
    GBM_GRM_MODES[grm]
end

function gbm_check(rc::Cint, what::String)
    rc == 0 && return nothing
    msg = what * ": " * gbm_last_error()
    rc == -1 ? throw(ArgumentError(msg)) : throw(ErrorException(msg))
end

"""
    gblup(; genomes, phenomes, idx_entries=nothing, idx_loci_alleles=nothing, idx_trait=1,
          verbose=false, λ=1.0, devices=Int32[], model_label="gblup", grm=:dropin)::Fit

GBLUP / RR-BLUP on V = G + λI with G = ZZᵀ/q, fitted on MI355X GPUs through libgbm.so.
Same keywords and Fit assembly as `ridge` (src/linear.jl:162-239), so it runs unchanged under
`cvbulk`/`cvmultithread!` (src/cross_validation.jl:170-177) and `predict`.
`λ = :reml` chooses λ = σ²_e/σ²_u by REML on the fit's own GRM first (gbm_gblup_fit_reml: the
reference's loglikreml objective, src/gwas.jl:450-483, over gwasreml's box, :577-590); a partial
of `gblup` with `λ = :reml` (e.g. `gblup_reml(; kw...) = gblup(; kw..., λ = :reml)`) then goes into
`cvbulk(models = [...])` unchanged.
`grm = :auto` computes the GRM exactly on the int8 matrix cores when the allele frequencies
are diploid dosages/2 (the usual `Genomes` of a diploid population; ≈3× faster at n = 5 000 and exact up to
each locus weight's fp64 rounding), else with the fp64-MFMA SYRK; `:fp64` / `:exact` force one. The default
`grm = :dropin` is `:auto` unless the environment sets GBM_GRM (fp64 | exact | auto), which then decides.
"""
function gblup(;
    genomes::Genomes,
    phenomes::Phenomes,
    idx_entries::Union{Nothing,Vector{Int64}} = nothing,
    idx_loci_alleles::Union{Nothing,Vector{Int64}} = nothing,
    idx_trait::Int64 = 1,
    verbose::Bool = false,
    λ::Union{Float64,Symbol} = 1.0,
    devices::Vector{Int32} = Int32[],
    model_label::String = "gblup",
    grm::Symbol = :dropin,
)::Fit
    X, y, entries, populations, loci_alleles = extractxyetc(
        genomes,
        phenomes,
        idx_entries = idx_entries,
        idx_loci_alleles = idx_loci_alleles,
        idx_trait = idx_trait,
        add_intercept = false,
    )
    n, p = size(X)
    fit::Fit = Fit(n = n, l = p)
    fit.model = model_label
    fit.b_hat_labels = vcat(["intercept"], loci_alleles)
    fit.trait = phenomes.traits[idx_trait]
    fit.entries = entries
    fit.populations = populations
    fit.y_true = y
    b_hat = zeros(p + 1)
    y_pred = zeros(n)
    mu = zeros(1)
    q = zeros(Int64, 1)
    λ_used = zeros(1)
    σ2 = zeros(2)
    grm_used = Cint[-1]
    mode = gbm_grm_mode(grm)
    devs = isempty(devices) ? C_NULL : pointer(devices)
    GC.@preserve X y b_hat y_pred mu q devices λ_used σ2 grm_used begin
        if λ isa Symbol
            λ === :reml || throw(ArgumentError("λ must be a Float64 or :reml, got :$λ"))
            rc = ccall(
                (:gbm_gblup_fit_reml_ex, LIBGBM),
                Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int32}, Cint, Cint,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Cint}),
                X, n, p, stride(X, 2), y, n, 1, devs, length(devices), mode,
                b_hat, y_pred, mu, q, λ_used, pointer(σ2, 1), pointer(σ2, 2), grm_used,
            )
            gbm_check(rc, "gblup (REML)")
        else
            rc = ccall(
                (:gbm_gblup_fit_ex, LIBGBM),
                Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64,
                 Ptr{Int32}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cint}),
                X, n, p, stride(X, 2), y, n, 1, λ,
                devs, length(devices), mode,
                b_hat, y_pred, mu, q, grm_used,
            )
            gbm_check(rc, "gblup")
            λ_used[1] = λ
        end
    end
    fit.b_hat = b_hat
    fit.y_pred = y_pred
    fit.metrics = metrics(y, y_pred)
    if verbose
        println("gblup: n=$n p=$p q=$(q[1]) μ̂=$(mu[1]) λ=$(λ_used[1]) grm=$(grm_used[1] == 1 ? "exact" : "fp64")" *
                (λ isa Symbol ? " (REML: σ²_e=$(σ2[1]), σ²_u=$(σ2[2]))" : ""))
        println(fit.metrics)
    end
    if !checkdims(fit)
        throw(ErrorException("Error fitting " * fit.model * "."))
    end
    fit
end

# ---- GWAS scans on the GPU (gbm_session_gwas; untested here like the rest of this file: no Julia in the
# build container; the Python mirror gbm/gwas.py drives the same ccall) -------------------------------------
# Both build the Fit with the reference's own gwasprep (src/gwas.jl:77-142) and replace the per-marker loop.
# Differences from the reference loops, stated in include/gbm.h: the variance components are estimated once
# under the null model (not per marker), K = ZZᵀ/q (not the column-standardised GRM), and the mixed model
# runs on that simple GRM only (GRM_type = "ploidy-aware" is refused by gwasreml_gpu).
# Leading k eigenpairs of the relationship matrix of the rows idx (0-based) of the session h (gbm_session_pcs):
# kind 0 = K = ZZᵀ/q, kind 1 = the PCA of the column-standardised K that gwasols takes PC1 from (src/gwas.jl:130,234).
# data_error = :nothing returns nothing instead of throwing when the library reports GBM_E_DATA (-7: the block lost
# rank, i.e. fewer than 32 eigenvalues above rounding, or a column of K without variance), for callers with a host path.
function gbm_session_pcs(h::Ptr{Cvoid}, idx::Vector{Int64}, k::Integer; kind::Integer = 0, tol::Float64 = 1e-10,
                         max_iter::Integer = 1000, data_error::Symbol = :throw)
    n = length(idx)
    vectors = zeros(n, k)
    values = zeros(k)
    resid = zeros(k)
    tr = zeros(1)
    iters = zeros(Int64, 1)
    rc = ccall((:gbm_session_pcs, LIBGBM), Cint,
               (Ptr{Cvoid}, Ptr{Int64}, Int64, Cint, Int64, Float64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Int64}),
               h, idx, n, kind, k, tol, max_iter, vectors, values, tr, resid, iters)
    rc == -7 && data_error == :nothing && return nothing
    gbm_check(rc, "pcs")
    converged = !startswith(gbm_last_error(), "warning:")
    (vectors = vectors, values = values, trace = tr[1], resid = resid, iters = iters[1], converged = converged)
end

# pc1 = :device: the scan's covariate is PC1 of the session's own cached GRM (kind 1, tol 1e-12; C is ignored); the
# result's pc1_found says whether the iteration converged (otherwise, and when the library reports a data error such
# as a block that lost rank, no scan was run and the caller falls back).
function gbm_gwas_scan(G::Matrix{Float64}, y::Vector{Float64}, C::Matrix{Float64}, model::Integer; device::Integer = 0,
                       pc1::Symbol = :given)
    n, p = size(G)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    gbm_check(ccall((:gbm_session_create, LIBGBM), Cint,
                    (Ptr{Float64}, Int64, Int64, Int64, Cint, Ptr{Ptr{Cvoid}}), G, n, p, n, device, h),
              "gwas (session)")
    z = zeros(p)
    b = zeros(p)
    σ2 = zeros(2)
    tested = zeros(Int64, 1)
    idx = collect(Int64, 0:(n-1))
    found = true
    try
        if pc1 == :device
            r = gbm_session_pcs(h[], idx, 1; kind = 1, tol = 1e-12, data_error = :nothing)
            found = !isnothing(r) && r.converged
            found && (C = r.vectors)
        end
        kc = size(C, 2)
        if found
            gbm_check(ccall((:gbm_session_gwas, LIBGBM), Cint,
                            (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Cint, Float64, Float64,
                             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                            h[], idx, n, y, kc > 0 ? C : Ptr{Float64}(C_NULL), n, kc, model, NaN, NaN, z, b, σ2, tested),
                      "gwas")
        end
    finally
        ccall((:gbm_session_destroy, LIBGBM), Cvoid, (Ptr{Cvoid},), h[])
    end
    (z = z, b = b, σ2_e = σ2[1], σ2_u = σ2[2], tested = tested[1], pc1_found = found)
end

"""
    gwasreml_gpu(; genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, GRM_type="simple", verbose=false)::Fit

`gwasreml` (src/gwas.jl:485-620) with the marker loop on the GPU: one null-model REML, one Cholesky, then
z_j for every locus from rows whitened against that factor.
"""
function gwasreml_gpu(; genomes::Genomes, phenomes::Phenomes, idx_entries = nothing, idx_loci_alleles = nothing,
                      idx_trait::Int64 = 1, GRM_type::String = "simple", verbose::Bool = false)::Fit
    GRM_type == "simple" || throw(ArgumentError("gwasreml_gpu runs on the simple GRM (ZZᵀ/q) only"))
    G, y, _, fit = gwasprep(genomes = genomes, phenomes = phenomes, idx_entries = idx_entries,
                            idx_loci_alleles = idx_loci_alleles, idx_trait = idx_trait, GRM_type = GRM_type,
                            standardise = true, verbose = false)
    r = gbm_gwas_scan(G, y, zeros(size(G, 1), 0), 0)
    fit.model = "GWAS_REML"
    fit.b_hat = r.z   # gwasprep already dropped the loci without variance: every column of G is kept
    verbose && println("gwasreml_gpu: tested=$(r.tested) σ²_e=$(r.σ2_e) σ²_u=$(r.σ2_u)")
    checkdims(fit) || throw(ErrorException("Error performing GWAS via REML on the GPU."))
    fit
end

"""
    gwasols_gpu(; genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, GRM_type="simple", pc="auto", verbose=false)::Fit

`gwasols` (src/gwas.jl:146-260) with the marker loop on the GPU. `pc = "auto"` with the simple GRM: PC1 comes from the
scan's own session on the device (`gbm_session_pcs`, the reference's PCA of the column-standardised GRM; one GRM
build, no n² transfer), and the host path is the fallback when the iteration does not converge, when the library
reports a data error (the block lost rank: fewer than about 31 polymorphic loci-alleles) or there are fewer than 64
entries. `pc = "host"`, and the ploidy-aware GRM always: PC1 of the GRM `gwasprep` returns, computed on the
host exactly as the reference does (src/gwas.jl:234).
"""
function gwasols_gpu(; genomes::Genomes, phenomes::Phenomes, idx_entries = nothing, idx_loci_alleles = nothing,
                     idx_trait::Int64 = 1, GRM_type::String = "simple", pc::String = "auto", verbose::Bool = false)::Fit
    pc in ("auto", "host") || throw(ArgumentError("Unrecognised `pc`. Please select from: auto, host"))
    G, y, GRM, fit = gwasprep(genomes = genomes, phenomes = phenomes, idx_entries = idx_entries,
                              idx_loci_alleles = idx_loci_alleles, idx_trait = idx_trait, GRM_type = GRM_type,
                              standardise = true, verbose = false)
    r = nothing
    if pc == "auto" && GRM_type == "simple" && size(G, 1) >= 64
        r = gbm_gwas_scan(G, y, zeros(size(G, 1), 0), 1; pc1 = :device)
        r.pc1_found || (r = nothing)
    end
    if isnothing(r)
        E = MultivariateStats.fit(PCA, GRM; maxoutdim = 1)
        r = gbm_gwas_scan(G, y, reshape(E.proj[:, 1], :, 1), 1)
    end
    fit.model = "GWAS_OLS"
    fit.b_hat = r.z
    verbose && println("gwasols_gpu: tested=$(r.tested)")
    checkdims(fit) || throw(ErrorException("Error performing GWAS via OLS on the GPU."))
    fit
end

# ---- lasso on the GPU (gbm_session_enet_path; untested here like the rest of this file: no Julia in the
# build container; the Python mirror gbm/linear.py `lasso` drives the same ccall) --------------------------
# One elastic-net path call on the rows idx (0-based) of the session h: (b_path (p+1) x nl_done, pred, nl_done).
function gbm_enet_path(h::Ptr{Cvoid}, p::Integer, idx::Vector{Int64}, y::Vector{Float64}, λ::Vector{Float64};
                       alpha::Float64 = 1.0, tol::Float64 = 1e-7, max_passes::Int64 = 1_000_000,
                       idx_eval::Vector{Int64} = Int64[], early_stop::Bool = true)
    nl = length(λ)
    path = zeros(p + 1, nl)
    pred = zeros(length(idx_eval), nl)
    done = zeros(Int64, 1)
    dev_max, fdev = early_stop ? (0.999, 1e-5) : (Inf, 0.0)
    GC.@preserve idx y λ path pred idx_eval done begin
        gbm_check(ccall((:gbm_session_enet_path, LIBGBM), Cint,
                        (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Int64, Float64, Int64,
                         Float64, Float64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64},
                         Ptr{Int64}, Ptr{Int64}),
                        h, idx, length(idx), y, alpha, λ, nl, tol, max_passes, dev_max, fdev, path,
                        isempty(idx_eval) ? Ptr{Int64}(C_NULL) : pointer(idx_eval), length(idx_eval),
                        isempty(idx_eval) ? Ptr{Float64}(C_NULL) : pointer(pred), done, C_NULL, C_NULL, C_NULL),
                  "enet_path")
    end
    msg = gbm_last_error()
    startswith(msg, "warning:") && @warn msg
    k = done[1]
    (path = path[:, 1:k], pred = pred[:, 1:k], nl_done = k)
end

"""
    lasso_gpu(; genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, verbose=false)::Fit

`lasso` (src/linear.jl:302-378) with `GLMNet.glmnetcv(alpha = 1.0, standardize = false, nlambda = 100,
lambda_min_ratio = 0.01, tol = 1e-7, intercept = true)` replaced by the coordinate-descent path on the GPU:
the full-data path with glmnet's early stop, GLMNet.jl's folds at the λ kept with the stop off, the mean
squared error per λ, then the reference's own selection loop (src/linear.jl:352-360) and Fit assembly.
"""
function lasso_gpu(; genomes::Genomes, phenomes::Phenomes, idx_entries = nothing, idx_loci_alleles = nothing,
                   idx_trait::Int64 = 1, verbose::Bool = false, device::Integer = 0)::Fit
    X, y, entries, populations, loci_alleles = extractxyetc(genomes, phenomes, idx_entries = idx_entries,
                                                            idx_loci_alleles = idx_loci_alleles, idx_trait = idx_trait,
                                                            add_intercept = false)
    n, p = size(X)
    fit = Fit(n = n, l = p)
    fit.model = "lasso"
    fit.b_hat_labels = vcat(["intercept"], loci_alleles)
    fit.trait = phenomes.traits[idx_trait]
    fit.entries = entries
    fit.populations = populations
    fit.y_true = y
    h = Ref{Ptr{Cvoid}}(C_NULL)
    gbm_check(ccall((:gbm_session_create, LIBGBM), Cint,
                    (Ptr{Float64}, Int64, Int64, Int64, Cint, Ptr{Ptr{Cvoid}}), X, n, p, n, device, h),
              "lasso (session)")
    local a0, betas, meanloss
    try
        all = collect(Int64, 0:(n-1))
        lmax = Ref(0.0)
        gbm_check(ccall((:gbm_session_ridge_lambda_max, LIBGBM), Cint,
                        (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}), h[], all, n, y, lmax),
                  "ridge_lambda_max")
        λ = collect((lmax[] * 1e-3) .* 0.01 .^ ((0:99) ./ 99))  # alpha = 1: glmnet's λ_max is the alpha = 0 one · 1e-3
        full = gbm_enet_path(h[], p, all, y, λ)
        λ = λ[1:full.nl_done]
        nfolds = min(10, div(n, 3))
        q, r = divrem(n, nfolds)
        folds = shuffle!([repeat(1:nfolds, outer = q); 1:r])  # GLMNet.jl's default folds
        loss = zeros(length(λ), nfolds)
        for f = 1:nfolds
            tr = findall(folds .!= f) .- 1
            ho = findall(folds .== f) .- 1
            res = gbm_enet_path(h[], p, tr, y[tr .+ 1], λ; idx_eval = ho, early_stop = false)
            loss[:, f] = vec(mean((res.pred .- y[ho .+ 1]) .^ 2, dims = 1))
        end
        a0, betas, meanloss = full.path[1, :], full.path[2:end, :], vec(mean(loss, dims = 2))
    finally
        ccall((:gbm_session_destroy, LIBGBM), Cvoid, (Ptr{Cvoid},), h[])
    end
    verbose && println(string("argmin = ", argmin(meanloss)))
    # Use the coefficients with variance (src/linear.jl:352-360)
    b_hat::Vector{Float64} = zeros(p + 1)
    idx_sort = sortperm(meanloss)
    INTERCEPTSs = a0[idx_sort]
    BETAs = betas[:, idx_sort]
    i = 1
    while var(b_hat[2:end]) < 1e-10
        b_hat = vcat(INTERCEPTSs[i], BETAs[:, i])
        i += 1
    end
    y_pred::Vector{Float64} = b_hat[1] .+ (X * b_hat[2:end])
    fit.b_hat = b_hat
    fit.metrics = metrics(y, y_pred)
    fit.y_pred = y_pred
    verbose && println(fit.metrics)
    checkdims(fit) || throw(ErrorException("Error fitting " * fit.model * "."))
    fit
end
