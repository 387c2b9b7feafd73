# NGPAutoGP.jl — Julia-side binding of libngp (include/ngp.h) behind the AutoGP surface that
# NowcastAutoGP calls (src/make_and_fit_model.jl:84-91, src/forecasting.jl:46-155).
#
# STATUS: written against include/ngp.h, NEVER EXECUTED — no `julia` binary exists in the build
# container or on the GPU box.  What IS checked mechanically (tests/test_julia_shim.py, CPU suite):
# every `ccall((:ngp_…` below against the header (symbol, arity, C type of every argument and of
# the result), the field lists of the mirrored structs, the presence of the thirteen AutoGP surface
# symbols the reference touches (SURVEY.md Appendix A), and that `Dict(::GPModel)` / `GPModel(::Dict)`
# use the keys of the version-1 wire format (nowcastautogp_amd/wire.py).  The Python package
# `nowcastautogp_amd` is the executed, tested host-side mirror of the same surface over the same
# C-ABI; the sampler moves here restate its design (nowcastautogp_amd/autogp.py).
module NGPAutoGP

using Dates, Random, LinearAlgebra

const LIBNGP = get(ENV, "LIBNGP", joinpath(@__DIR__, "..", "nowcastautogp_amd", "libngp.so"))

# ---- include/ngp.h mirrors --------------------------------------------------------------------
struct NgpSpec              # ngp_spec
    se_form::Int32
    periodic_form::Int32
    cp_form::Int32
    precision::Int32
    jitter::Float64
    mixed_tau::Float64
    refine_tol::Float64
    refine_max::Int32
    reserved::Int32
end
default_spec(; precision = 0) = NgpSpec(0, 0, 0, precision, 1.0e-5, 1.0e-6, 1.0e-9, 3, 0)

struct NgpKernel            # ngp_kernel
    n_ops::Int32
    n_params::Int32
    ops::Ptr{Int32}
    params::Ptr{Float64}
    noise::Float64
end

struct NgpError <: Exception
    status::Int32
    where::String
end
Base.showerror(io::IO, e::NgpError) = print(io, e.where, ": ",
    unsafe_string(ccall((:ngp_strerror, LIBNGP), Cstring, (Int32,), e.status)), " (", e.status, ")")

check(st, where) = st == 0 ? nothing : throw(NgpError(st, where))

mutable struct Context
    h::Ptr{Cvoid}
    function Context(device::Integer = 0)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ngp_ctx_create, LIBNGP), Int32, (Int32, Ref{Ptr{Cvoid}}), device, r),
              "ngp_ctx_create")
        c = new(r[])
        finalizer(x -> ccall((:ngp_ctx_destroy, LIBNGP), Cvoid, (Ptr{Cvoid},), x.h), c)
        return c
    end
end

function set_spec(c::Context, s::NgpSpec)
    check(ccall((:ngp_set_spec, LIBNGP), Int32, (Ptr{Cvoid}, Ref{NgpSpec}), c.h, Ref(s)),
          "ngp_set_spec")
end
function get_spec(c::Context)
    r = Ref(default_spec())
    check(ccall((:ngp_get_spec, LIBNGP), Int32, (Ptr{Cvoid}, Ref{NgpSpec}), c.h, r), "ngp_get_spec")
    return r[]
end

const _default_ctx = Ref{Union{Nothing, Context}}(nothing)
default_context() = (_default_ctx[] === nothing && (_default_ctx[] = Context(0)); _default_ctx[])

# One particle's kernel as the postfix arrays the ABI carries; opcodes follow
# AutoGP.GP.GPConfig (Constant=1 ... ChangePoint=8).
struct Program
    ops::Vector{Int32}
    params::Vector{Float64}
    noise::Float64
end

"GC-safe view of a vector of programs as an array of ngp_kernel (keep `progs` alive via GC.@preserve)."
kernels(progs::Vector{Program}) = [NgpKernel(length(p.ops), length(p.params), pointer(p.ops),
                                             pointer(p.params), p.noise) for p in progs]

function kernel_check(p::Program)
    GC.@preserve p begin
        k = Ref(NgpKernel(length(p.ops), length(p.params), pointer(p.ops), pointer(p.params), p.noise))
        return ccall((:ngp_kernel_check, LIBNGP), Int32, (Ref{NgpKernel},), k) == 0
    end
end

# ---- entry points -------------------------------------------------------------------------------
function logml_batch(c::Context, progs::Vector{Program}, t::Vector{Float64}, y::VecOrMat{Float64})
    B, n = length(progs), length(t)
    ldy = y isa Vector ? 0 : n            # Matrix y is n x B column-major == [B x n] row-major
    out, info = Vector{Float64}(undef, B), zeros(Int32, B)
    GC.@preserve progs begin
        ks = kernels(progs)
        check(ccall((:ngp_logml_batch, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Int32}),
                    c.h, B, ks, n, t, y, ldy, out, info), "ngp_logml_batch")
    end
    return out, info
end

"""
Concurrent callers (include/ngp.h): one-shot calls entered from several tasks at once — the
`Threads.@spawn` per scenario of the reference's `forecast_with_nowcasts`, src/forecasting.jl:131-159
— are combined inside libngp into one launch sequence per group of compatible requests.  On by
default; `set_combining(ctx, false)` makes every call wait for the context and run alone.
`combine_stats(ctx)` = (requests, launch sequences, largest group, requests that shared one, requests
served from one shared factorisation per particle).
"""
set_combining(c::Context, on::Bool) =
    check(ccall((:ngp_set_combining, LIBNGP), Int32, (Ptr{Cvoid}, Int32), c.h, on), "ngp_set_combining")
"an item's outputs no longer depend, in their last bits, on the batch it travels in (include/ngp.h)"
set_batch_invariant(c::Context, on::Bool) =
    check(ccall((:ngp_set_batch_invariant, LIBNGP), Int32, (Ptr{Cvoid}, Int32), c.h, on),
          "ngp_set_batch_invariant")
"series whose main block is at most 256 points factorised in one launch (on by default; include/ngp.h)"
set_short_series_path(c::Context, on::Bool) =
    check(ccall((:ngp_set_short_series_path, LIBNGP), Int32, (Ptr{Cvoid}, Int32), c.h, on),
          "ngp_set_short_series_path")
function combine_stats(c::Context; reset::Bool = false)
    out = zeros(Int64, 6)
    check(ccall((:ngp_combine_stats, LIBNGP), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int32), c.h, out, reset),
          "ngp_combine_stats")
    return (requests = out[1], sequences = out[2], largest_group = out[3], shared = out[4],
            shared_k = out[5])
end

"storage option of staged value jobs (include/ngp.h): results are bit-identical either way"
set_structured_storage(c::Context, on::Bool) =
    check(ccall((:ngp_set_structured_storage, LIBNGP), Int32, (Ptr{Cvoid}, Int32), c.h, on),
          "ngp_set_structured_storage")

function logml_grad_batch(c::Context, progs::Vector{Program}, t::Vector{Float64},
                          y::VecOrMat{Float64})
    B, n = length(progs), length(t)
    ldy = y isa Vector ? 0 : n
    sizes = [length(p.params) + 1 for p in progs]
    grad = Vector{Float64}(undef, sum(sizes))
    lm, info = Vector{Float64}(undef, B), zeros(Int32, B)
    GC.@preserve progs begin
        ks = kernels(progs)
        check(ccall((:ngp_logml_grad_batch, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    c.h, B, ks, n, t, y, ldy, lm, grad, info), "ngp_logml_grad_batch")
    end
    offs = cumsum([0; sizes])
    return lm, [grad[offs[i]+1:offs[i+1]] for i in 1:B], info
end

"""
A gradient job whose trees, dates and observations stay on the device (include/ngp.h
`ngp_grad_stage`): the leapfrog steps of one HMC move change nothing but the parameters, so per
step only they cross the bus.  `run!(job, progs)` evaluates logml and gradient for the parameters
`progs` hold now (the same trees, in the same order); `close(job)` releases it.
"""
mutable struct GradJob
    h::Ptr{Cvoid}
    sizes::Vector{Int}
end

function grad_stage(c::Context, progs::Vector{Program}, t::Vector{Float64}, y::VecOrMat{Float64})
    B, n = length(progs), length(t)
    ldy = y isa Vector ? 0 : n
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve progs begin
        ks = kernels(progs)
        check(ccall((:ngp_grad_stage, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64}, Int64,
                     Ptr{Ptr{Cvoid}}),
                    c.h, B, ks, n, t, y, ldy, h), "ngp_grad_stage")
    end
    job = GradJob(h[], [length(p.params) + 1 for p in progs])
    finalizer(close, job)
    return job
end

function run!(job::GradJob, progs::Union{Nothing,Vector{Program}} = nothing)
    B = length(job.sizes)
    if progs !== nothing
        flat = reduce(vcat, [p.params for p in progs]; init = Float64[])
        noise = Float64[p.noise for p in progs]
        check(ccall((:ngp_grad_job_set_params, LIBNGP), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                    job.h, flat, noise), "ngp_grad_job_set_params")
    end
    grad = Vector{Float64}(undef, sum(job.sizes))
    lm, info = Vector{Float64}(undef, B), zeros(Int32, B)
    check(ccall((:ngp_grad_job_run, LIBNGP), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                job.h, lm, grad, info), "ngp_grad_job_run")
    offs = cumsum([0; job.sizes])
    return lm, [grad[offs[i]+1:offs[i+1]] for i in 1:B], info
end

"`ngp_hmc_config` of include/ngp.h: the prior entries are indexed by latent kind (0 real, 1 unit,
2 gamma, 3 period, 4 wildcard)."
struct NgpHmcConfig
    n_leapfrog::Int32
    eps::Float64
    prior_mu::NTuple{5,Float64}
    prior_sigma::NTuple{5,Float64}
end

const KIND_CODE = Dict(:real => 0x00, :unit => 0x01, :gamma => 0x02, :period => 0x03, :wildcard => 0x04)

"""
    hmc!(job, kinds, z0, mom, n_leapfrog, eps, prior; frozen = nothing)

`ngp_grad_job_hmc`: one whole leapfrog trajectory of every item of the staged job in ONE call
(n_leapfrog + 1 gradient evaluations, the update between them on the device).  `kinds` (UInt8,
`KIND_CODE`), `z0`, `mom`, `frozen` hold one entry per latent: an item's parameters in program
order, then its noise, items back to back.  The library draws nothing: momenta and the accept
decision stay here.  Returns a named tuple (z1, mom1, theta1, U0, K0, U1, K1, logml1, info1).
"""
function hmc!(job::GradJob, kinds::Vector{UInt8}, z0::Vector{Float64}, mom::Vector{Float64},
              n_leapfrog::Int, eps::Float64, prior; frozen::Union{Nothing,Vector{UInt8}} = nothing)
    B, NL = length(job.sizes), sum(job.sizes)
    @assert length(kinds) == NL && length(z0) == NL && length(mom) == NL
    mu(k) = Float64(prior[k][:mu]); sg(k) = Float64(prior[k][:sigma])
    cfg = Ref(NgpHmcConfig(Int32(n_leapfrog), eps,
                           (0.0, 0.0, mu(:gamma), mu(:period), mu(:wildcard)),
                           (1.0, 1.0, sg(:gamma), sg(:period), sg(:wildcard))))
    z1, mom1, theta1 = (Vector{Float64}(undef, NL) for _ in 1:3)
    U0, K0, U1, K1, lm1 = (Vector{Float64}(undef, B) for _ in 1:5)
    info1 = zeros(Int32, B)
    fr = frozen === nothing ? UInt8[] : frozen
    GC.@preserve cfg kinds fr begin
        check(ccall((:ngp_grad_job_hmc, LIBNGP), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                    job.h, Base.unsafe_convert(Ptr{Cvoid}, cfg), pointer(kinds),
                    frozen === nothing ? C_NULL : pointer(fr), z0, mom, z1, mom1, theta1, U0, K0, U1, K1,
                    lm1, info1, C_NULL), "ngp_grad_job_hmc")
    end
    return (; z1, mom1, theta1, U0, K0, U1, K1, logml1 = lm1, info1)
end

function Base.close(job::GradJob)
    if job.h != C_NULL
        ccall((:ngp_grad_job_destroy, LIBNGP), Cvoid, (Ptr{Cvoid},), job.h)
        job.h = C_NULL
    end
    return nothing
end

function predict_batch(c::Context, progs::Vector{Program}, t::Vector{Float64},
                       y::VecOrMat{Float64}, t_new::Vector{Float64}; noise_on_new::Bool = true)
    B, n, m = length(progs), length(t), length(t_new)
    ldy = y isa Vector ? 0 : n
    mu = Matrix{Float64}(undef, m, B)             # column b = item b  (row-major [B x m])
    sigma = Array{Float64}(undef, m, m, B)        # symmetric per item: layout-agnostic
    lm, info = Vector{Float64}(undef, B), zeros(Int32, B)
    GC.@preserve progs begin
        ks = kernels(progs)
        check(ccall((:ngp_predict_batch, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64}, Int64,
                     Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    c.h, B, ks, n, t, y, ldy, m, t_new, noise_on_new, mu, sigma, lm, info),
              "ngp_predict_batch")
    end
    return mu, sigma, lm, info
end

"add_data! + predict_mvn for ALL scenarios of ALL particles in one call (src/forecasting.jl:133-155)."
function nowcast_batch(c::Context, progs::Vector{Program}, t::Vector{Float64}, y::Vector{Float64},
                       t_add::Vector{Float64}, y_add::Matrix{Float64},  # d x D (column = scenario)
                       t_new::Vector{Float64}; noise_on_new::Bool = true)
    P, n, d, D, m = length(progs), length(t), length(t_add), size(y_add, 2), length(t_new)
    lb, lf = Vector{Float64}(undef, P), Matrix{Float64}(undef, D, P)
    mu = Array{Float64}(undef, m, D, P)
    sigma = Array{Float64}(undef, m, m, P)
    info = zeros(Int32, P)
    GC.@preserve progs begin
        ks = kernels(progs)
        check(ccall((:ngp_nowcast_batch, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64}, Int32,
                     Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    c.h, P, ks, n, t, y, d, t_add, D, y_add, m, t_new, noise_on_new, lb, lf, mu,
                    sigma, info), "ngp_nowcast_batch")
    end
    return (logml_base = lb, logml_full = lf, mu = mu, sigma = sigma, info = info)
end

"""
Resident factor (include/ngp.h `ngp_factor_*`): factorise the ensemble on its training data once,
then every `predict_mvn` / `add_data!` fan-out on the same fitted model only sweeps its own rows
through the L kept on the device.
"""
mutable struct Factor
    h::Ptr{Cvoid}
    P::Int
    ctx::Context            # keeps the context alive for as long as the handle
    function Factor(c::Context, progs::Vector{Program}, t::Vector{Float64}, y::VecOrMat{Float64})
        r = Ref{Ptr{Cvoid}}(C_NULL)
        n = length(t)
        ldy = y isa Vector ? 0 : n
        GC.@preserve progs begin
            ks = kernels(progs)
            check(ccall((:ngp_factor_create, LIBNGP), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64}, Int64,
                         Ref{Ptr{Cvoid}}), c.h, length(progs), ks, n, t, y, ldy, r),
                  "ngp_factor_create")
        end
        f = new(r[], length(progs), c)
        finalizer(x -> ccall((:ngp_factor_destroy, LIBNGP), Cvoid, (Ptr{Cvoid},), x.h), f)
        return f
    end
end

function nowcast(f::Factor, t_add::Vector{Float64}, y_add::Matrix{Float64}, t_new::Vector{Float64};
                 noise_on_new::Bool = true)
    P, d, D, m = f.P, length(t_add), max(size(y_add, 2), 1), length(t_new)
    lb, lf = Vector{Float64}(undef, P), Matrix{Float64}(undef, D, P)
    mu = Array{Float64}(undef, m, D, P)
    sigma = Array{Float64}(undef, m, m, P)
    info = zeros(Int32, P)
    check(ccall((:ngp_factor_nowcast, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                f.h, d, t_add, D, y_add, m, t_new, noise_on_new, lb, lf, mu, sigma, info),
          "ngp_factor_nowcast")
    return (logml_base = lb, logml_full = lf, mu = mu, sigma = sigma, info = info)
end

"""
One query for a horizon of up to `NGP_MAX_LONG_HORIZON` dates (include/ngp.h
`ngp_factor_predict_long`): the dates are the panel of a triangular solve against the resident
factor, not aux rows, so `horizon_room` does not bound them.  `t_add` / `y_add` as `nowcast`
(empty: plain predict).  Without `want_sigma` no m x m array is formed.  No weight update:
`nowcast` with no dates gives it.
"""
function predict_long(f::Factor, t_new::Vector{Float64};
                      t_add::Vector{Float64} = Float64[],
                      y_add::Matrix{Float64} = Matrix{Float64}(undef, 0, 1),
                      noise_on_new::Bool = true, want_sigma::Bool = true)
    P, d, D, m = f.P, length(t_add), max(size(y_add, 2), 1), length(t_new)
    mu = Array{Float64}(undef, m, D, P)
    var = Matrix{Float64}(undef, m, P)
    sigma = want_sigma ? Array{Float64}(undef, m, m, P) : nothing
    info = zeros(Int32, P)
    check(ccall((:ngp_factor_predict_long, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                f.h, d, t_add, D, y_add, m, t_new, noise_on_new, mu, var,
                want_sigma ? pointer(sigma) : Ptr{Float64}(C_NULL), info),
          "ngp_factor_predict_long")
    return (mu = mu, var = var, sigma = sigma, info = info)
end

"""
Hindcasts from the resident factor (include/ngp.h `ngp_factor_predict_origins`): origin r knows the
first `cuts[r]` observations (strictly increasing, 1 .. n).  One query: the means and variances are
running sums along the solved panel rows of `predict_long`, no factorisation per origin.  Returns
`mu`, `var` (m x R x P), `logml` (R x P: log p(y_1:cuts[r])) and `info` (P).
"""
function predict_origins(f::Factor, cuts::Vector{Int32}, t_new::Vector{Float64};
                         noise_on_new::Bool = true)
    P, R, m = f.P, length(cuts), length(t_new)
    mu = Array{Float64}(undef, m, R, P)
    var = Array{Float64}(undef, m, R, P)
    logml = Matrix{Float64}(undef, R, P)
    info = zeros(Int32, P)
    check(ccall((:ngp_factor_predict_origins, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                f.h, R, cuts, m, t_new, noise_on_new, mu, var, logml, info),
          "ngp_factor_predict_origins")
    return (mu = mu, var = var, logml = logml, info = info)
end

"""
Paths of a long horizon drawn on the device (include/ngp.h `ngp_factor_sample_long`): the mixtures
`w` (P x S, S = number of scenarios, 1 without appended points) over the components `predict_long`
returns for the same query, under the contract of `mixture_sample`.  sigma never leaves the device.
Returns `out` (m x draws x S), `comp` (draws x S, 0-based), `info` and `chol_info` (P); a path picked
from a particle with `info > 0` or `chol_info > 0` is NaN.
"""
function sample_long(f::Factor, t_new::Vector{Float64}, w::Matrix{Float64}, draws::Integer,
                     seed::UInt64;
                     t_add::Vector{Float64} = Float64[],
                     y_add::Matrix{Float64} = Matrix{Float64}(undef, 0, 1),
                     noise_on_new::Bool = true)
    P, d, D, m = f.P, length(t_add), max(size(y_add, 2), 1), length(t_new)
    size(w) == (P, D) || throw(ArgumentError("w must be P x S"))
    out = Array{Float64}(undef, m, draws, D)
    comp = Matrix{Int32}(undef, draws, D)
    info = zeros(Int32, P)
    chol_info = zeros(Int32, P)
    check(ccall((:ngp_factor_sample_long, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32,
                 Ptr{Float64}, Int32, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}, Ptr{Int32}),
                f.h, d, t_add, D, y_add, m, t_new, noise_on_new, w, draws, seed, out, comp,
                Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), info, chol_info),
          "ngp_factor_sample_long")
    return (out = out, comp = comp, info = info, chol_info = chol_info)
end

"""
Paths of a long horizon from independent mixtures (include/ngp.h `ngp_factor_sample_long_indep`):
the factor's P items are S mixtures of P' = P / S components each, mixture-major (item s P' + k is
component k of mixture s; a refined scenario clone holds its nowcast points as data).  `w` is
P' x S, `seeds` has one key per mixture; mixture s draws what `sample_long` draws on a factor of its
own items with `seeds[s]`.  Returns `out` (m x draws x S), `comp` (draws x S, 0-based within the
mixture), `info` and `chol_info` (P); a path picked from an item with `info > 0` or `chol_info > 0`
is NaN.
"""
function sample_long_indep(f::Factor, t_new::Vector{Float64}, w::Matrix{Float64}, draws::Integer,
                           seeds::Vector{UInt64}; noise_on_new::Bool = true)
    P, S, m = f.P, length(seeds), length(t_new)
    (S >= 1 && P % S == 0) || throw(ArgumentError("the factor's items must be S mixtures of equal size"))
    size(w) == (P ÷ S, S) || throw(ArgumentError("w must be P' x S"))
    out = Array{Float64}(undef, m, draws, S)
    comp = Matrix{Int32}(undef, draws, S)
    info = zeros(Int32, P)
    chol_info = zeros(Int32, P)
    check(ccall((:ngp_factor_sample_long_indep, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{UInt64},
                 Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                f.h, S, m, t_new, noise_on_new, w, draws, seeds, out, comp,
                Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), info, chol_info),
          "ngp_factor_sample_long_indep")
    return (out = out, comp = comp, info = info, chol_info = chol_info)
end

"""
The additive components of a program (include/ngp.h `ngp_kernel_components`): the maximal non-Plus
subtrees under the root's Plus nodes, left to right, each a `Program` of its own.
"""
function kernel_components(p::Program)
    cap = length(p.ops) ÷ 2 + 1
    cnt = Ref{Int32}(0)
    of, ol, pf, pl = zeros(Int32, cap), zeros(Int32, cap), zeros(Int32, cap), zeros(Int32, cap)
    GC.@preserve p begin
        k = Ref(NgpKernel(length(p.ops), length(p.params), pointer(p.ops), pointer(p.params), p.noise))
        check(ccall((:ngp_kernel_components, LIBNGP), Int32,
                    (Ref{NgpKernel}, Ref{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                    k, cnt, of, ol, pf, pl), "ngp_kernel_components")
    end
    return [Program(p.ops[of[i]+1:of[i]+ol[i]], p.params[pf[i]+1:pf[i]+pl[i]], p.noise) for i in 1:cnt[]]
end

"""
Joint posterior of every particle's additive parts on the dates `t_new` (include/ngp.h
`ngp_factor_components`): `comps[p]` are particle p's component programs.  Returns per particle
`mu` (m x C_p), `var` (m x C_p) and `sigma` (C_p m x C_p m, index = (c - 1) m + j); the C_p m rows
share the aux block: (n mod 64) + 1 + C_p m <= NGP_MAX_AUX.
"""
function components(f::Factor, comps::Vector{Vector{Program}}, t_new::Vector{Float64})
    length(comps) == f.P || throw(ArgumentError("one vector of component programs per particle"))
    m = length(t_new)
    counts = Int32[length(c) for c in comps]
    flat = reduce(vcat, comps)
    tot = length(flat)
    mu, var = Matrix{Float64}(undef, m, tot), Matrix{Float64}(undef, m, tot)
    sizes = [(Int(c) * m)^2 for c in counts]
    sg = Vector{Float64}(undef, sum(sizes))
    info = zeros(Int32, f.P)
    GC.@preserve flat begin
        ks = kernels(flat)
        check(ccall((:ngp_factor_components, LIBNGP), Int32,
                    (Ptr{Cvoid}, Ptr{Int32}, Ptr{NgpKernel}, Int32, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    f.h, counts, ks, m, t_new, mu, sg, var, info), "ngp_factor_components")
    end
    first = cumsum(vcat(0, Int.(counts))); soff = cumsum(vcat(0, sizes))
    return (mu = [mu[:, first[p]+1:first[p+1]] for p in 1:f.P],
            var = [var[:, first[p]+1:first[p+1]] for p in 1:f.P],
            sigma = [reshape(sg[soff[p]+1:soff[p+1]], Int(counts[p]) * m, Int(counts[p]) * m) for p in 1:f.P],
            info = info)
end

const NGP_SPLIT_PLUS, NGP_SPLIT_CHANGEPOINT, NGP_SPLIT_TIMES = Int32(0), Int32(1), Int32(2)

"""
The sum-of-products terms of a program (include/ngp.h `ngp_kernel_terms`): new `Program`s that sum
to it.  `split`: NGP_SPLIT_* flags or-ed (0: the programs of `kernel_components`); a ChangePoint is
split into its two windows, each blended against Constant(0), a Times distributed over the sums
below it.  More than `max_terms` terms is an error (NGP_ERR_TOO_LARGE).
"""
function kernel_terms(p::Program, split::Integer; max_terms::Integer = typemax(Int32))
    cnt = Ref{Int32}(0)
    GC.@preserve p begin
        k = Ref(NgpKernel(length(p.ops), length(p.params), pointer(p.ops), pointer(p.params), p.noise))
        check(ccall((:ngp_kernel_terms, LIBNGP), Int32,
                    (Ref{NgpKernel}, Int32, Int32, Ref{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                     Ptr{Int32}, Int32, Ptr{Float64}, Int32),
                    k, split, max_terms, cnt, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 0, C_NULL, 0),
              "ngp_kernel_terms")
        n = Int(cnt[])
        of, ol, pf, pl = zeros(Int32, n), zeros(Int32, n), zeros(Int32, n), zeros(Int32, n)
        ops, par = zeros(Int32, n * length(p.ops)), zeros(Float64, n * length(p.params))
        check(ccall((:ngp_kernel_terms, LIBNGP), Int32,
                    (Ref{NgpKernel}, Int32, Int32, Ref{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                     Ptr{Int32}, Int32, Ptr{Float64}, Int32),
                    k, split, n, cnt, of, ol, pf, pl, ops, length(ops), par, length(par)),
              "ngp_kernel_terms")
        return [Program(ops[of[i]+1:of[i]+ol[i]], par[pf[i]+1:pf[i]+pl[i]], p.noise) for i in 1:n]
    end
end

"""
`components` conditioned on the appended points `t_add` (d) and the scenarios `y_add` (d x D)
(include/ngp.h `ngp_factor_components_nowcast`).  Returns per particle `mu` (m x D x C_p), `var`
(m x C_p) and `sigma` (C_p m x C_p m), shared by the scenarios, and `logml_full` (D x P);
(n mod 64) + d + 1 + C_p m <= NGP_MAX_AUX.
"""
function components_nowcast(f::Factor, comps::Vector{Vector{Program}}, t_add::Vector{Float64},
                            y_add::Matrix{Float64}, t_new::Vector{Float64})
    length(comps) == f.P || throw(ArgumentError("one vector of component programs per particle"))
    d, D, m = length(t_add), max(size(y_add, 2), 1), length(t_new)
    counts = Int32[length(c) for c in comps]
    flat = reduce(vcat, comps)
    tot = length(flat)
    mu, var = Array{Float64}(undef, m, D, tot), Matrix{Float64}(undef, m, tot)
    sizes = [(Int(c) * m)^2 for c in counts]
    sg = Vector{Float64}(undef, sum(sizes))
    lf = Matrix{Float64}(undef, D, f.P)
    info = zeros(Int32, f.P)
    GC.@preserve flat begin
        ks = kernels(flat)
        check(ccall((:ngp_factor_components_nowcast, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{NgpKernel}, Int32,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    f.h, d, t_add, D, y_add, counts, ks, m, t_new, lf, mu, sg, var, info),
              "ngp_factor_components_nowcast")
    end
    first = cumsum(vcat(0, Int.(counts))); soff = cumsum(vcat(0, sizes))
    return (mu = [mu[:, :, first[p]+1:first[p+1]] for p in 1:f.P],
            var = [var[:, first[p]+1:first[p+1]] for p in 1:f.P],
            sigma = [reshape(sg[soff[p]+1:soff[p+1]], Int(counts[p]) * m, Int(counts[p]) * m) for p in 1:f.P],
            logml_full = lf, info = info)
end

"""
`components_nowcast` over a horizon of up to `NGP_MAX_LONG_HORIZON` dates in ONE query (include/ngp.h
`ngp_factor_components_long`): the component rows are groups of the panel of `predict_long`'s solve,
not aux rows.  `t_add` / `y_add` as `predict_long` (empty: no appended points).  Returns per particle
`mu` (m x S x C_p), `cross` (m x C_p x C_p: the covariance of two parts at the same date, its c = c'
planes the variances) and, with `want_sigma`, `sigma` (C_p m x C_p m); without it nothing of that size
is formed and `sigma` is `nothing`.
"""
function components_long(f::Factor, comps::Vector{Vector{Program}}, t_new::Vector{Float64};
                         t_add::Vector{Float64} = Float64[],
                         y_add::Matrix{Float64} = Matrix{Float64}(undef, 0, 1),
                         want_sigma::Bool = false)
    length(comps) == f.P || throw(ArgumentError("one vector of component programs per particle"))
    d, D, m = length(t_add), max(size(y_add, 2), 1), length(t_new)
    counts = Int32[length(c) for c in comps]
    flat = reduce(vcat, comps)
    mu = Array{Float64}(undef, m, D, length(flat))
    csz = [Int(c)^2 * m for c in counts]
    sizes = [(Int(c) * m)^2 for c in counts]
    cr = Vector{Float64}(undef, sum(csz))
    sg = want_sigma ? Vector{Float64}(undef, sum(sizes)) : nothing
    info = zeros(Int32, f.P)
    GC.@preserve flat begin
        ks = kernels(flat)
        check(ccall((:ngp_factor_components_long, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{NgpKernel}, Int32,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    f.h, d, t_add, D, y_add, counts, ks, m, t_new, mu, cr,
                    want_sigma ? pointer(sg) : Ptr{Float64}(C_NULL), info),
              "ngp_factor_components_long")
    end
    first = cumsum(vcat(0, Int.(counts))); coff = cumsum(vcat(0, csz)); soff = cumsum(vcat(0, sizes))
    return (mu = [mu[:, :, first[p]+1:first[p+1]] for p in 1:f.P],
            cross = [reshape(cr[coff[p]+1:coff[p+1]], m, Int(counts[p]), Int(counts[p])) for p in 1:f.P],
            sigma = want_sigma ? [reshape(sg[soff[p]+1:soff[p+1]], Int(counts[p]) * m, Int(counts[p]) * m)
                                  for p in 1:f.P] : nothing,
            info = info)
end

"Draws from S mixtures over the same components on the device (include/ngp.h `ngp_mixture_sample`)."
function mixture_sample(c::Context, w::Matrix{Float64},        # P x S  (column = scenario)
                        mu::Array{Float64,3},                   # m x S x P
                        sigma::Array{Float64,3},                # m x m x P
                        draws::Integer, seed::UInt64)
    P, S, m = size(w, 1), size(w, 2), size(mu, 1)
    out = Array{Float64}(undef, m, draws, S)
    info = zeros(Int32, P)
    check(ccall((:ngp_mixture_sample, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                 UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                c.h, P, S, m, w, mu, sigma, draws, seed, out, C_NULL, info), "ngp_mixture_sample")
    raise_if_not_posdef(info)
    return out
end

function weights_normalize(logw::Vector{Float64})
    w = similar(logw); ess = Ref(0.0); ln = Ref(0.0)
    check(ccall((:ngp_weights_normalize, LIBNGP), Int32,
                (Int32, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}),
                length(logw), logw, w, ess, ln), "ngp_weights_normalize")
    return w, ess[], ln[]
end

"Every COLUMN of a P x D log-weight matrix at once (include/ngp.h `ngp_weights_normalize_cols`): the D scenario clones."
function weights_normalize_cols(logw::Matrix{Float64})          # P x D, column = scenario
    P, D = size(logw)
    lw = permutedims(logw)                                      # D x P column-major == [P x D] row-major
    w = similar(lw); ess = Vector{Float64}(undef, D); ln = Vector{Float64}(undef, D)
    check(ccall((:ngp_weights_normalize_cols, LIBNGP), Int32,
                (Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                P, D, lw, w, ess, ln), "ngp_weights_normalize_cols")
    return permutedims(w), ess, ln
end

"S independent mixtures of P components each, one device call (include/ngp.h `ngp_mixture_sample_indep`)."
function mixture_sample_indep(c::Context, w::Matrix{Float64},        # P x S (column = mixture)
                              mu::Array{Float64,3},                   # m x P x S
                              sigma::Array{Float64,4},                # m x m x P x S
                              draws::Integer, seeds::Vector{UInt64})
    P, S, m = size(w, 1), size(w, 2), size(mu, 1)
    out = Array{Float64}(undef, m, draws, S)
    info = zeros(Int32, P, S)
    check(ccall((:ngp_mixture_sample_indep, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                 Ptr{UInt64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                c.h, P, S, m, w, mu, sigma, draws, seeds, out, C_NULL, info),
          "ngp_mixture_sample_indep")
    raise_if_not_posdef(vec(info))
    return out
end

# ---- exact summaries of a mixture's per-date marginals (include/ngp.h) --------------------------
# A mixture is C components over m dates: w [C], mu and var m x C (column = component, which is the
# header's [C x m] row-major).  A date whose info is c > 0 has a component (c, 1-based) with a
# non-finite mean or a variance that is not finite and positive; its outputs are NaN.
function _check_marginals(w::Vector{Float64}, mu::Matrix{Float64}, var::Matrix{Float64})
    size(mu) == size(var) && size(mu, 2) == length(w) ||
        throw(DimensionMismatch("w [C], mu and var m x C"))
    return size(mu, 2), size(mu, 1)
end

"F_j(x) of every date j at K points: x is m x K; returns (cdf m x K, info) (`ngp_mixture_cdf`). With x = y the PIT values."
function mixture_cdf(c::Context, w::Vector{Float64}, mu::Matrix{Float64}, var::Matrix{Float64},
                     x::Matrix{Float64})
    C, m = _check_marginals(w, mu, var)
    size(x, 1) == m || throw(DimensionMismatch("x is m x K"))
    K = size(x, 2)
    xt = permutedims(x)                                         # K x m column-major == [m x K] row-major
    out = similar(xt); info = zeros(Int32, m)
    check(ccall((:ngp_mixture_cdf, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                c.h, C, m, w, mu, var, K, xt, out, info), "ngp_mixture_cdf")
    return permutedims(out), info
end

"Exact quantiles per date, `quantile(dist, probs)` without draws: returns (q m x Q, info) (`ngp_mixture_quantiles`)."
function mixture_quantiles(c::Context, w::Vector{Float64}, mu::Matrix{Float64}, var::Matrix{Float64},
                           probs::Vector{Float64})
    C, m = _check_marginals(w, mu, var)
    Q = length(probs)
    out = Matrix{Float64}(undef, Q, m); info = zeros(Int32, m)
    check(ccall((:ngp_mixture_quantiles, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                c.h, C, m, w, mu, var, Q, probs, out, info), "ngp_mixture_quantiles")
    return permutedims(out), info
end

"Closed-form CRPS per date against y [m], on the scale of the mixture: returns (crps, info) (`ngp_mixture_crps`)."
function mixture_crps(c::Context, w::Vector{Float64}, mu::Matrix{Float64}, var::Matrix{Float64},
                      y::Vector{Float64})
    C, m = _check_marginals(w, mu, var)
    length(y) == m || throw(DimensionMismatch("y has one entry per date"))
    out = Vector{Float64}(undef, m); info = zeros(Int32, m)
    check(ccall((:ngp_mixture_crps, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Int32}),
                c.h, C, m, w, mu, var, y, out, info), "ngp_mixture_crps")
    return out, info
end

# ---- trajectory targets: functionals of whole sample paths (include/ngp.h) ----------------------
# Mirrors of ngp_inv_transform / ngp_path_target (C layout: Int32 then 8-byte aligned doubles).
struct InvTransform
    kind::Int32
    lam::Float64
    offset::Float64
    cap::Float64
end

const NGP_SCORE_NATURAL = Int32(0)
const NGP_SCORE_LOG = Int32(1)

"""
Exact CRPS and mean of the forecast after the inverse transformation `inv`, on the natural scale
(`scale = NGP_SCORE_NATURAL`) or on log(. + shift) (`NGP_SCORE_LOG`), against y [m] on the ORIGINAL
scale: returns (crps, mean, err, info) (`ngp_mixture_crps_mapped`); `tol <= 0`: the default.
"""
function mixture_crps_mapped(c::Context, w::Vector{Float64}, mu::Matrix{Float64}, var::Matrix{Float64},
                             inv::InvTransform, scale::Integer, shift::Real, y::Vector{Float64};
                             tol::Real = 0.0)
    C, m = _check_marginals(w, mu, var)
    length(y) == m || throw(DimensionMismatch("y has one entry per date"))
    out = Vector{Float64}(undef, m); mean = Vector{Float64}(undef, m); err = Vector{Float64}(undef, m)
    info = zeros(Int32, m)
    iv = Ref(inv)
    GC.@preserve iv check(ccall((:ngp_mixture_crps_mapped, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid},
                 Int32, Float64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}),
                c.h, C, m, w, mu, var, Base.unsafe_convert(Ptr{Cvoid}, iv), Int32(scale),
                Float64(shift), y, Float64(tol), out, mean, err, info), "ngp_mixture_crps_mapped")
    return out, mean, err, info
end
struct PathTarget
    kind::Int32
    j0::Int32        # 0-based, as the header: the window j0 .. j1 is inclusive
    j1::Int32
    thr::Float64
end
const INV_IDENTITY, INV_EXP, INV_LOGISTIC100, INV_BOXCOX = Int32(0), Int32(1), Int32(2), Int32(3)
const TARGET_SUM, TARGET_MAX, TARGET_DIFF, TARGET_ARGMAX, TARGET_EXCEED =
    Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)

"""
Summaries of functionals of the paths `mixture_sample` (one `seed`) / `mixture_sample_indep` (a
vector of S seeds) draws for the same arguments, on the scale `inv` maps to: returns
`(q Q x T, mean, count, hist m x T, values)` — `values` (N x T) only with `want_values = true`.
`w`, `mu`, `sigma` in the layouts of the two samplers (`ngp_mixture_path_targets[_indep]`).
"""
function mixture_path_targets(c::Context, w::Array{Float64}, mu::Array{Float64}, sigma::Array{Float64},
                              draws::Integer, seed::Union{Integer,Vector{UInt64}}, inv::InvTransform,
                              targets::Vector{PathTarget}, probs::Vector{Float64};
                              want_values::Bool = false)
    P, S, m = size(w, 1), size(w, 2), size(mu, 1)              # column-major views of [S x P], [.. x m]
    T, Q, N = length(targets), length(probs), S * Int(draws)
    q = Matrix{Float64}(undef, Q, T); mean = Vector{Float64}(undef, T)
    count = zeros(Int64, T); hist = zeros(Int64, m, T)
    values = want_values ? Matrix{Float64}(undef, N, T) : nothing
    vptr = want_values ? pointer(values) : Ptr{Float64}(C_NULL)
    rinv = Ref(inv)
    if seed isa Integer
        info = zeros(Int32, P)
        GC.@preserve values check(ccall((:ngp_mixture_path_targets, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                     UInt64, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
                    c.h, P, S, m, w, mu, sigma, draws, UInt64(seed), rinv, T, targets, Q, probs,
                    q, mean, count, hist, vptr, info), "ngp_mixture_path_targets")
    else
        length(seed) == S || throw(DimensionMismatch("one seed per mixture"))
        info = zeros(Int32, P * S)
        GC.@preserve values check(ccall((:ngp_mixture_path_targets_indep, LIBNGP), Int32,
                    (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                     Ptr{UInt64}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
                    c.h, P, S, m, w, mu, sigma, draws, seed, rinv, T, targets, Q, probs,
                    q, mean, count, hist, vptr, info), "ngp_mixture_path_targets_indep")
    end
    raise_if_not_posdef(vec(info))
    return q, mean, count, hist, values
end

"""
Energy score per window of dates of N paths (`ngp_ensemble_scores`): `x` is m x N (a column is a
path on the original scale, as `forecast` returns its draws), `y` has m entries, `win` is 2 x W with
the 0-based inclusive `j0, j1` of every window; a window of one date is the sample CRPS of that
date.  Returns `(es, term_obs, term_pair, info)`.
"""
function ensemble_scores(c::Context, x::Matrix{Float64}, y::Vector{Float64}, win::Matrix{Int32};
                         scale::Integer = NGP_SCORE_NATURAL, shift::Real = 0.0, fair::Bool = true)
    m, N = size(x)
    length(y) == m || throw(DimensionMismatch("y has one entry per date"))
    size(win, 1) == 2 || throw(DimensionMismatch("win is 2 x W"))
    W = size(win, 2)
    es = Vector{Float64}(undef, W); to = Vector{Float64}(undef, W); tp = Vector{Float64}(undef, W)
    info = zeros(Int32, W)
    check(ccall((:ngp_ensemble_scores, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32, Int32,
                 Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                c.h, N, m, x, y, Int32(scale), Float64(shift), Int32(fair), W, win, es, to, tp, info),
          "ngp_ensemble_scores")
    return es, to, tp, info
end

"""
The same scores of the paths `mixture_sample` (one `seed`) / `mixture_sample_indep` (a vector of S
seeds) draws for the same arguments, mapped through `inv` and scored on the device without coming
back (`ngp_mixture_path_scores`).  Returns `(es, term_obs, term_pair, info)`.
"""
function mixture_path_scores(c::Context, w::Array{Float64}, mu::Array{Float64}, sigma::Array{Float64},
                             draws::Integer, seed::Union{Integer,Vector{UInt64}}, inv::InvTransform,
                             y::Vector{Float64}, win::Matrix{Int32};
                             scale::Integer = NGP_SCORE_NATURAL, shift::Real = 0.0, fair::Bool = true)
    P, S, m = size(w, 1), size(w, 2), size(mu, 1)              # column-major views of [S x P], [.. x m]
    length(y) == m || throw(DimensionMismatch("y has one entry per date"))
    size(win, 1) == 2 || throw(DimensionMismatch("win is 2 x W"))
    indep = !(seed isa Integer)
    seeds = indep ? seed : UInt64[UInt64(seed)]
    indep && length(seeds) != S && throw(DimensionMismatch("one seed per mixture"))
    W = size(win, 2)
    es = Vector{Float64}(undef, W); to = Vector{Float64}(undef, W); tp = Vector{Float64}(undef, W)
    info = zeros(Int32, W); cinfo = zeros(Int32, indep ? P * S : P)
    rinv = Ref(inv)
    check(ccall((:ngp_mixture_path_scores, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32,
                 Ptr{UInt64}, Ptr{Cvoid}, Ptr{Float64}, Int32, Float64, Int32, Int32, Ptr{Int32},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                c.h, P, S, m, w, mu, sigma, Int32(indep), draws, seeds, rinv, y, Int32(scale),
                Float64(shift), Int32(fair), W, win, es, to, tp, info, cinfo),
          "ngp_mixture_path_scores")
    raise_if_not_posdef(cinfo)
    return es, to, tp, info
end

"""
The one collective of the path for a multi-GPU Julia host (one process per GPU): RCCL, opened by
libngp at run time.  Rank 0 calls `comm_unique_id()` and hands the 128 bytes to the other ranks by
whatever the host uses (Distributed.jl, MPI, a file); every rank then builds `Comm(ctx, id, rank, world)`.
"""
"(first, rows) of `rank` in the block partition of P_total particles over `world` ranks (0-based)."
function shard(P_total::Integer, world::Integer, rank::Integer)
    a = Ref{Int32}(0); b = Ref{Int32}(0)
    check(ccall((:ngp_shard, LIBNGP), Int32, (Int32, Int32, Int32, Ref{Int32}, Ref{Int32}),
                P_total, world, rank, a, b), "ngp_shard")
    return Int(a[]), Int(b[])
end
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    check(ccall((:ngp_comm_unique_id, LIBNGP), Int32, (Ptr{Cvoid},), id), "ngp_comm_unique_id")
    return id
end
mutable struct Comm
    h::Ptr{Cvoid}
    rank::Int
    world::Int
    ctx::Context
    function Comm(c::Context, id::Vector{UInt8}, rank::Integer, world::Integer)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ngp_comm_create, LIBNGP), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ref{Ptr{Cvoid}}), c.h, id, rank, world, r),
              "ngp_comm_create")
        m = new(r[], rank, world, c)
        finalizer(x -> ccall((:ngp_comm_destroy, LIBNGP), Cvoid, (Ptr{Cvoid},), x.h), m)
        return m
    end
end
"This rank's rows `logw_local` (P_local x D) -> (w_local, w_all, ess, log_norm) over ALL ranks' particles."
function weights_allgather_normalize(cm::Comm, logw_local::Matrix{Float64}, P_total::Integer)
    P_loc, D = size(logw_local)
    lw = permutedims(logw_local)
    w_loc = similar(lw); w_all = Matrix{Float64}(undef, D, P_total)
    ess = Vector{Float64}(undef, D); ln = Vector{Float64}(undef, D)
    check(ccall((:ngp_weights_allgather_normalize, LIBNGP), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}), cm.h, P_total, D, lw, w_loc, w_all, ess, ln),
          "ngp_weights_allgather_normalize")
    return permutedims(w_loc), permutedims(w_all), ess, ln
end

"""
The host half of that exchange for a host with its own all-gather (MPI.jl, Distributed): `padded` is
D x pmax x world (column-major; the row-major [world][pmax][D] the C side reads) — every rank's
zero-padded shard as gathered — and comes out as (w_all P_total x D, ess, log_norm).
"""
function weights_unpad_normalize(padded::Array{Float64,3}, P_total::Integer)
    D, _, world = size(padded)
    w_all = Matrix{Float64}(undef, D, P_total)
    ess = Vector{Float64}(undef, D); ln = Vector{Float64}(undef, D)
    check(ccall((:ngp_weights_unpad_normalize, LIBNGP), Int32,
                (Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                P_total, world, D, padded, w_all, ess, ln), "ngp_weights_unpad_normalize")
    return permutedims(w_all), ess, ln
end

"info[b] > 0  =>  PosDefException(info[b]), as the reference surfaces it (src/make_and_fit_model.jl:6-8)."
raise_if_not_posdef(info) = (k = findfirst(>(0), info); k === nothing || throw(PosDefException(info[k])))

# ---- kernel grammar: AutoGP.GP.GPConfig (src/NowcastAutoGP.jl:9; defaults as printed in
#      docs/src/vignettes/setting-priors.md:228-245) ------------------------------------------------
module GP
Base.@kwdef mutable struct GPConfig
    Constant::Int = 1
    Linear::Int = 2
    SquaredExponential::Int = 3
    GammaExponential::Int = 4
    Periodic::Int = 5
    Plus::Int = 6
    Times::Int = 7
    ChangePoint::Int = 8
    node_dist_leaf::Vector{Float64} = [0.0, 1 / 3, 0.0, 1 / 3, 1 / 3]
    node_dist_nocp::Vector{Float64} = [0.0, 3 / 14, 0.0, 3 / 14, 3 / 14, 5 / 28, 5 / 28]
    node_dist_cp::Vector{Float64} = [0.0, 3 / 14, 0.0, 3 / 14, 3 / 14, 1 / 7, 1 / 7, 1 / 14]
    max_branch::Int = 2
    max_depth::Int = -1
    changepoints::Bool = true
    noise::Union{Nothing, Float64} = nothing
    prior::Dict{Symbol, Dict{Symbol, Float64}} = Dict(
        :gamma => Dict(:mu => 0.0, :sigma => 1.0),
        :period => Dict(:mu => -1.5, :sigma => 1.0),
        :wildcard => Dict(:mu => -1.5, :sigma => 1.0))
end
end # module GP
const GPConfig = GP.GPConfig

const N_PARAMS = (1, 3, 2, 3, 3, 0, 0, 2)               # per opcode 1..8
# kind of every parameter, per opcode: :real, :unit, :gamma, :period, :wildcard
const PARAM_KINDS = ((:wildcard,), (:real, :wildcard, :wildcard), (:wildcard, :wildcard),
                     (:wildcard, :gamma, :wildcard), (:wildcard, :period, :wildcard), (), (),
                     (:unit, :wildcard))

mutable struct Node
    op::Int
    params::Vector{Float64}
    left::Union{Nothing, Node}
    right::Union{Nothing, Node}
end
isleaf(n::Node) = n.op < 6
treesize(n::Node) = isleaf(n) ? 1 : 1 + treesize(n.left) + treesize(n.right)

_sigmoid(x) = x >= 0 ? 1 / (1 + exp(-min(x, 700.0))) : (e = exp(max(x, -700.0)); e / (1 + e))
"latent z ~ N(0,1) -> parameter and d theta / d z (nowcastautogp_amd/gp.py transform)"
function transform(z::Float64, kind::Symbol, prior)
    if kind === :real
        return z, 1.0
    elseif kind === :unit
        s = _sigmoid(z); return s, s * (1 - s)
    elseif kind === :gamma
        pr = prior[:gamma]; s = _sigmoid(pr[:mu] + pr[:sigma] * z)
        return 2s, 2s * (1 - s) * pr[:sigma]
    else
        pr = kind === :period ? prior[:period] : prior[:wildcard]
        v = exp(clamp(pr[:mu] + pr[:sigma] * z, -300.0, 300.0))
        return v, v * pr[:sigma]
    end
end
function untransform(th::Float64, kind::Symbol, prior)
    kind === :real && return th
    # strictly inside the open domain of the kind: a saturated value (gamma == 2.0, unit == 1.0,
    # a positive parameter == 0) has an infinite latent and would freeze its particle
    th = kind === :unit ? clamp(th, 1.0e-9, 1.0 - 1.0e-9) :
         kind === :gamma ? clamp(th, 1.0e-9, 2.0 - 1.0e-9) : max(th, 1.0e-12)
    kind === :unit && return log(th / (1 - th))
    if kind === :gamma
        pr = prior[:gamma]; s = th / 2
        return (log(s / (1 - s)) - pr[:mu]) / pr[:sigma]
    end
    pr = kind === :period ? prior[:period] : prior[:wildcard]
    return (log(th) - pr[:mu]) / pr[:sigma]
end

function _categorical(rng, p)
    u = rand(rng); c = 0.0
    for (i, pi) in enumerate(p)
        c += pi
        u < c && return i
    end
    return length(p)
end

"Draw a kernel tree from the grammar prior (parameters from their priors)."
function sample_tree(rng, cfg::GPConfig, depth::Int = 1; depth_cap::Int = 6)
    cap = cfg.max_depth > 0 ? cfg.max_depth : depth_cap
    dist = depth >= cap ? cfg.node_dist_leaf : (cfg.changepoints ? cfg.node_dist_cp : cfg.node_dist_nocp)
    op = _categorical(rng, dist)
    th = [transform(randn(rng), k, cfg.prior)[1] for k in PARAM_KINDS[op]]
    op < 6 && return Node(op, th, nothing, nothing)
    l = sample_tree(rng, cfg, depth + 1; depth_cap)
    r = sample_tree(rng, cfg, depth + 1; depth_cap)
    return Node(op, th, l, r)
end
sample_noise(rng, cfg::GPConfig) =
    cfg.noise === nothing ? transform(randn(rng), :wildcard, cfg.prior)[1] : cfg.noise

function to_program(n::Node, noise::Float64)
    ops = Int32[]; params = Float64[]
    walk(nd) = (isleaf(nd) || (walk(nd.left); walk(nd.right)); push!(ops, nd.op); append!(params, nd.params))
    walk(n)
    return Program(ops, params, noise)
end
function from_program(p::Program)
    stack = Node[]; k = 0
    for op in p.ops
        np = N_PARAMS[op]; th = p.params[k+1:k+np]; k += np
        if op < 6
            push!(stack, Node(op, th, nothing, nothing))
        else
            r = pop!(stack); l = pop!(stack)
            push!(stack, Node(op, th, l, r))
        end
    end
    return only(stack)
end
param_kinds(p::Program) = Symbol[k for op in p.ops for k in PARAM_KINDS[op]]

# ---- the AutoGP surface NowcastAutoGP touches (SURVEY.md Appendix A) ----------------------------
mutable struct GPModel
    config::GPConfig
    ds::Vector{Date}
    y::Vector{Float64}
    particles::Vector{Program}
    log_weights::Vector{Float64}
    logml::Vector{Float64}          # log p(y[perm[1:n_obs]] | particle)
    n_obs::Int
    perm::Vector{Int}               # data-annealing order (1-based here, 0-based on the wire)
    ds_slope::Float64               # model time = ds_slope * days + ds_intercept
    ds_intercept::Float64
    y_slope::Float64                # model y = y_slope * y + y_intercept
    y_intercept::Float64
    depth_cap::Int
    rng::AbstractRNG
    ctx::Context
    n_particles_total::Int          # over all ranks (== length(particles) on one GPU)
end
GPModel(cfg, ds, y, parts, lw, lm, n_obs, perm, dss, dsi, ys, yi, cap, rng, ctx) =
    GPModel(cfg, ds, y, parts, lw, lm, n_obs, perm, dss, dsi, ys, yi, cap, rng, ctx, length(parts))
num_particles(m::GPModel) = m.n_particles_total

_days(ds) = Float64[Dates.value(d) for d in ds]

"AutoGP.GPModel(ds, y; n_particles, config) — src/make_and_fit_model.jl:84-87"
function GPModel(ds::AbstractVector{<:Dates.TimeType}, y::AbstractVector{<:Real};
                 n_particles::Int = 8, config::GPConfig = GPConfig(),
                 ctx::Context = default_context(), rng::AbstractRNG = Random.default_rng(),
                 depth_cap::Int = 6)
    length(ds) == length(y) || throw(ArgumentError("ds and y must have the same length"))
    days = _days(ds); lo, hi = extrema(days); span = hi > lo ? hi - lo : 1.0
    ylo, yhi = extrema(y)
    yhi > ylo || throw(PosDefException(1))     # flat series: src/make_and_fit_model.jl:6-8
    ys = 2 / (yhi - ylo)
    parts = [to_program(sample_tree(rng, config; depth_cap), sample_noise(rng, config))
             for _ in 1:n_particles]
    return GPModel(config, collect(Date, ds), collect(Float64, y), parts, zeros(n_particles),
                   zeros(n_particles), 0, collect(1:length(y)), 1 / span, -lo / span, ys,
                   -ys * (yhi + ylo) / 2, depth_cap, rng, ctx)
end

"""
Model time of dates: `slope * (days - origin)`.  The subtraction of day numbers is exact, so dates
whole days apart land on an exact lattice — which the library needs to replace the transcendentals
of the kernel grammar by table lookups; `slope * days + intercept` on day numbers of ~7e5 loses
eleven digits to cancellation (nowcastautogp_amd/autogp.py `DateTransform`).
"""
function _model_time(m::GPModel, ds)
    o = -m.ds_intercept / m.ds_slope
    abs(o - round(o)) < 1.0e-6 && (o = round(o))
    return m.ds_slope .* (_days(ds) .- o)
end

function _obs(m::GPModel, count::Int = m.n_obs)
    idx = sort(m.perm[1:count])
    return _model_time(m, m.ds[idx]), m.y_slope .* m.y[idx] .+ m.y_intercept
end

module Schedule
"Cumulative observation counts of the data-annealing steps (src/make_and_fit_model.jl:90)."
function linear_schedule(n::Int, percent::Float64)
    step = max(1, round(Int, percent * n))
    out = collect(step:step:n-1)
    push!(out, n)
    return out
end
end # module Schedule

function _refresh_logml(m::GPModel, count::Int)
    t, y = _obs(m, count)
    lm, info = logml_batch(m.ctx, m.particles, t, y)
    return [(info[i] != 0 || !isfinite(lm[i])) ? -Inf : lm[i] for i in eachindex(lm)]
end
_advance(lw, new, old) = [isinf(n) && n < 0 ? -Inf : (v = w + (n - o); isnan(v) ? -Inf : v)
                          for (w, n, o) in zip(lw, new, old)]

# ---- lockstep: the D scenario clones of forecast_with_nowcasts (src/forecasting.jl:131-159) advance
#      together — every proposal / leapfrog / prediction is ONE call of P x D items with per-item y
#      rows (ldy = n), instead of D tasks entering the library one after another.  Model j draws
#      from its own `rng` in the order the single-model functions do, so the result is that of the
#      per-scenario loop for the same seeds.  The single-model functions are the D = 1 case. ----
"(t, Y): shared model times and the per-item observation rows (n x B, column = item)."
function _group_obs(ms::Vector{GPModel})
    t, y1 = _obs(ms[1])
    ys = [y1]
    for m in ms[2:end]
        tj, yj = _obs(m)
        (length(tj) == length(t) && tj == t) ||
            throw(ArgumentError("models advanced in lockstep must share their observation dates"))
        push!(ys, yj)
    end
    return t, ys
end
_item_y(ys, owner) = length(ys) == 1 ? ys[1] : reduce(hcat, (ys[j] for j in owner))

function _structure_move!(ms::Vector{GPModel}, t, ys)
    props = Program[]; idx = Tuple{Int, Int}[]
    for (j, m) in enumerate(ms), (k, p) in enumerate(m.particles)
        tree = from_program(p)
        nodes = Tuple{Node, Int, Union{Nothing, Node}, Symbol}[]
        walk(nd, depth, parent, side) = (push!(nodes, (nd, depth, parent, side));
            isleaf(nd) || (walk(nd.left, depth + 1, nd, :left); walk(nd.right, depth + 1, nd, :right)))
        walk(tree, 1, nothing, :root)
        nd, depth, parent, side = nodes[rand(m.rng, 1:length(nodes))]
        sub = sample_tree(m.rng, m.config, depth; depth_cap = m.depth_cap)
        new = parent === nothing ? sub : (setfield!(parent, side, sub); tree)
        prog = to_program(new, p.noise)
        kernel_check(prog) || continue
        push!(props, prog); push!(idx, (j, k))
    end
    isempty(props) && return 0
    lm, info = logml_batch(ms[1].ctx, props, t, _item_y(ys, [j for (j, _) in idx]))
    acc = 0
    for (i, (j, k)) in enumerate(idx)
        (info[i] != 0 || !isfinite(lm[i])) && continue
        m = ms[j]
        log_a = (lm[i] - m.logml[k]) + log(length(m.particles[k].ops) / length(props[i].ops))
        if log(rand(m.rng)) < log_a
            m.particles[k] = props[i]; m.logml[k] = lm[i]; acc += 1
        end
    end
    return acc
end
_structure_move!(m::GPModel, t, y) = _structure_move!([m], t, [y])

"One HMC transition per particle of every model on the N(0,1) latents of (parameters, noise)."
function _hmc_move!(ms::Vector{GPModel}, t, ys, n_leapfrog::Int, eps::Float64)
    prior = ms[1].config.prior
    fixed_noise = ms[1].config.noise !== nothing
    items = [(j, k) for (j, m) in enumerate(ms) for k in 1:length(m.particles)]
    B = length(items)
    parts = [ms[j].particles[k] for (j, k) in items]
    Y = _item_y(ys, [j for (j, _) in items])
    kinds = [vcat(param_kinds(p), [:wildcard]) for p in parts]
    z0 = [[untransform(th, k, prior) for (th, k) in zip(vcat(p.params, p.noise), kd)]
          for (p, kd) in zip(parts, kinds)]
    job = nothing      # staged at the first evaluation: trees, dates, observations go up once per move
    function potential(z)
        progs = Program[]; dths = Vector{Float64}[]
        for (p, kd, zk) in zip(parts, kinds, z)
            td = [transform(clamp(isnan(v) ? 0.0 : v, -50.0, 50.0), k, prior) for (v, k) in zip(zk, kd)]
            th = [clamp(a[1], -1.0e6, 1.0e6) for a in td]
            push!(dths, [a[2] for a in td])
            push!(progs, Program(p.ops, th[1:end-1], max(th[end], 1.0e-12)))
        end
        if job === nothing
            job = grad_stage(ms[1].ctx, progs, t, Y)
            lm, grads, info = run!(job)                                # ONE call of P x D items
        else
            lm, grads, info = run!(job, progs)                         # new parameters, nothing else
        end
        U = similar(lm); dU = Vector{Float64}[]
        for i in 1:B
            ok = info[i] == 0 && isfinite(lm[i]) && all(isfinite, grads[i])
            U[i] = ok ? -lm[i] + 0.5 * sum(abs2, z[i]) : Inf
            g = ok ? (-grads[i] .* dths[i] .+ z[i]) : zeros(length(z[i]))
            fixed_noise && (g[end] = 0.0)
            push!(dU, g)
        end
        return U, dU, lm, progs
    end
    local H0, U1, lm1, progs1, pm
    try
        U0, dU, _, _ = potential(z0)
        mom = [randn(ms[j].rng, length(z0[i])) for (i, (j, _)) in enumerate(items)]
        fixed_noise && foreach(p -> (p[end] = 0.0), mom)
        H0 = [U0[i] + 0.5 * sum(abs2, mom[i]) for i in 1:B]
        z = deepcopy(z0)
        pm = [mom[i] .- 0.5 * eps .* dU[i] for i in 1:B]
        U1 = U0; lm1 = zeros(B); progs1 = parts
        for step in 1:n_leapfrog
            z = [z[i] .+ eps .* pm[i] for i in 1:B]
            U1, dU, lm1, progs1 = potential(z)
            h = step < n_leapfrog ? eps : 0.5 * eps
            pm = [pm[i] .- h .* dU[i] for i in 1:B]
        end
    finally
        job === nothing || close(job)     # the device arena goes back whatever a step threw
    end
    acc = 0
    for (i, (j, k)) in enumerate(items)
        H1 = U1[i] + 0.5 * sum(abs2, pm[i])
        u = rand(ms[j].rng)
        if isfinite(H1) && log(u) < H0[i] - H1
            ms[j].particles[k] = progs1[i]; ms[j].logml[k] = lm1[i]; acc += 1
        end
    end
    return acc
end
_hmc_move!(m::GPModel, t, y, n_leapfrog::Int, eps::Float64) = _hmc_move!([m], t, [y], n_leapfrog, eps)

"The transition with the whole trajectory in ONE library call (`hmc!`, ngp_grad_job_hmc): one `ccall`
per move instead of one per leapfrog.  Momenta and accept uniforms are drawn here, from the same
generators in the same order as `_hmc_move!`.  The arithmetic is the LIBRARY's, i.e. the Python
mirror's `potential` (include/ngp.h): z = +-Inf is evaluated as +-50, theta is kept inside the gamma
and unit margins (1e-9) as well as above 1e-12, and the installed parameters are those clipped
values.  `_hmc_move!` above clamps z to +-50 and only the noise from below, so the two paths of the
shim agree where no clamp bites (every ordinary move) and differ at the margins."
function _hmc_move_device!(ms::Vector{GPModel}, t, ys, n_leapfrog::Int, eps::Float64)
    prior = ms[1].config.prior
    fixed_noise = ms[1].config.noise !== nothing
    items = [(j, k) for (j, m) in enumerate(ms) for k in 1:length(m.particles)]
    parts = [ms[j].particles[k] for (j, k) in items]
    Y = _item_y(ys, [j for (j, _) in items])
    kinds = [vcat(param_kinds(p), [:wildcard]) for p in parts]
    z0 = [[untransform(th, k, prior) for (th, k) in zip(vcat(p.params, p.noise), kd)]
          for (p, kd) in zip(parts, kinds)]
    mom = [randn(ms[j].rng, length(z0[i])) for (i, (j, _)) in enumerate(items)]
    fixed_noise && foreach(p -> (p[end] = 0.0), mom)
    frozen = nothing
    if fixed_noise
        frozen = reduce(vcat, [vcat(zeros(UInt8, length(z) - 1), 0x01) for z in z0])
    end
    codes = UInt8[KIND_CODE[k] for kd in kinds for k in kd]
    dev = grad_stage(ms[1].ctx, parts, t, Y)
    local out
    try
        out = hmc!(dev, codes, reduce(vcat, z0), reduce(vcat, mom), n_leapfrog, eps, prior; frozen)
    finally
        close(dev)
    end
    offs = cumsum([0; dev.sizes])
    acc = 0
    for (i, (j, k)) in enumerate(items)
        H0, H1 = out.U0[i] + out.K0[i], out.U1[i] + out.K1[i]
        u = rand(ms[j].rng)
        if isfinite(H1) && log(u) < H0 - H1
            th = out.theta1[offs[i]+1:offs[i+1]]
            ms[j].particles[k] = Program(parts[i].ops, th[1:end-1], th[end])
            ms[j].logml[k] = out.logml1[i]; acc += 1
        end
    end
    return acc
end

"`hmc_config` may carry `device = true`: every move is then one call of ngp_grad_job_hmc."
_hmc_step!(ms, t, ys, cfg) = get(cfg, :device, false) ?
    _hmc_move_device!(ms, t, ys, cfg.n_leapfrog, cfg.eps) : _hmc_move!(ms, t, ys, cfg.n_leapfrog, cfg.eps)

const DEFAULT_HMC = (n_leapfrog = 10, eps = 0.02, device = false)

"AutoGP.mcmc_parameters!(model, n_hmc) — src/forecasting.jl:65, 148"
function mcmc_parameters!(m::GPModel, n_hmc::Int; hmc_config = DEFAULT_HMC)
    mcmc_parameters_lockstep!([m], n_hmc; hmc_config)
    return m
end
function mcmc_parameters_lockstep!(ms::Vector{GPModel}, n_hmc::Int; hmc_config = DEFAULT_HMC)
    t, ys = _group_obs(ms)
    for _ in 1:n_hmc
        _hmc_step!(ms, t, ys, hmc_config)
    end
    return ms
end

"AutoGP.mcmc_structure!(model, n_mcmc, n_hmc) — src/forecasting.jl:146"
function mcmc_structure!(m::GPModel, n_mcmc::Int, n_hmc::Int; hmc_config = DEFAULT_HMC)
    mcmc_structure_lockstep!([m], n_mcmc, n_hmc; hmc_config)
    return m
end
function mcmc_structure_lockstep!(ms::Vector{GPModel}, n_mcmc::Int, n_hmc::Int;
                                  hmc_config = DEFAULT_HMC)
    t, ys = _group_obs(ms)
    for _ in 1:n_mcmc
        _structure_move!(ms, t, ys)
        for _ in 1:n_hmc
            _hmc_step!(ms, t, ys, hmc_config)
        end
    end
    return ms
end

"AutoGP.maybe_resample!(model, ess) — src/forecasting.jl:138-141 (absolute ESS threshold)"
function maybe_resample!(m::GPModel, ess_threshold::Real)
    return maybe_resample_lockstep!([m], ess_threshold)[1]
end
"""
D models at once: ONE normalisation call for all weight vectors (`ngp_weights_normalize_cols`;
`comm`: one RCCL all-gather over the ranks' particle shards, `ngp_weights_allgather_normalize`).
In a multi-GPU host every rank draws the same ancestors (same `rng` state on every rank) and
rebuilds its shard from the descriptors the host exchanges — no matrix ever moves.
"""
function maybe_resample_lockstep!(ms::Vector{GPModel}, ess_threshold::Real;
                                  comm::Union{Nothing, Comm} = nothing)
    logw = reduce(hcat, (m.log_weights for m in ms))               # P_local x D
    if comm === nothing
        w, ess, _ = weights_normalize_cols(logw)
    else
        P_total = ms[1].n_particles_total
        _, w, ess, _ = weights_allgather_normalize(comm, logw, P_total)
        comm.world == 1 || error("multi-rank resampling: exchange the particle descriptors " *
                                 "(ops, params, noise, logml) between ranks in the host, then rebuild " *
                                 "this rank's shard from ancestors[shard] as below")
    end
    done = falses(length(ms))
    for (j, m) in enumerate(ms)
        ess[j] < ess_threshold || continue
        cw = cumsum(w[:, j])
        anc = [min(searchsortedfirst(cw, rand(m.rng)), length(cw)) for _ in 1:length(cw)]
        m.particles = m.particles[anc]; m.logml = m.logml[anc]; fill!(m.log_weights, 0.0)
        done[j] = true
    end
    return done
end

"""
AutoGP.fit_smc!(model; schedule, n_mcmc, n_hmc, kwargs...) — src/make_and_fit_model.jl:91.
`n_mcmc` and `n_hmc` have no defaults: omitting them is an UndefKeywordError, as in AutoGP
(test/test_gpconfig.jl:42).
"""
function fit_smc!(m::GPModel; schedule, n_mcmc::Int, n_hmc::Int, hmc_config = DEFAULT_HMC,
                  biased::Bool = false, shuffle::Bool = true, adaptive_resampling::Bool = true,
                  adaptive_rejuvenation::Bool = false, verbose::Bool = false)
    n = length(m.y)
    m.perm = shuffle ? randperm(m.rng, n) : collect(1:n)
    P = num_particles(m)
    for count in schedule
        count = min(count, n)
        count <= m.n_obs && continue
        lm = _refresh_logml(m, count)
        m.log_weights = _advance(m.log_weights, lm, m.logml)
        m.logml = lm
        m.n_obs = count
        resampled = maybe_resample!(m, adaptive_resampling ? P / 2 : Inf)
        (!adaptive_rejuvenation || resampled) && mcmc_structure!(m, n_mcmc, n_hmc; hmc_config)
        verbose && @info "fit_smc!" n_obs = count
    end
    return m
end

"AutoGP.add_data!(model, ds, y) — src/forecasting.jl:135"
function add_data!(m::GPModel, ds::AbstractVector{<:Dates.TimeType}, y::AbstractVector{<:Real})
    length(ds) == length(y) || throw(ArgumentError("ds and y must have the same length"))
    m.n_obs == length(m.y) || error("add_data! on a model that has not absorbed all of its data")
    n_old = length(m.y)
    append!(m.ds, ds); append!(m.y, y); append!(m.perm, n_old+1:n_old+length(y))
    lm = _refresh_logml(m, length(m.y))
    m.log_weights = _advance(m.log_weights, lm, m.logml)
    m.logml = lm
    m.n_obs = length(m.y)
    return m
end

"""
`add_data!` on D clones of `base` at once: the appended covariance rows do not depend on the
scenario, so all D weight updates are ONE query of the base model's factor (P factorisations at
most — `ngp_nowcast_batch`, or none with a resident `Factor`), not P x D.
"""
function add_data_lockstep!(ms::Vector{GPModel}, ds::AbstractVector{<:Dates.TimeType},
                            ys::Vector{<:AbstractVector{<:Real}}, base::GPModel;
                            factor::Union{Nothing, Factor} = nothing)
    length(ys) == length(ms) && all(length(y) == length(ds) for y in ys) ||
        throw(ArgumentError("one vector of length(ds) observations per model"))
    t, y = _obs(base)
    t_add = _model_time(base, ds)
    y_add = reduce(hcat, (base.y_slope .* Float64.(v) .+ base.y_intercept for v in ys))   # d x D
    o = factor === nothing ? nowcast_batch(base.ctx, base.particles, t, y, t_add, y_add, Float64[]) :
                             nowcast(factor, t_add, y_add, Float64[])
    for (j, m) in enumerate(ms)
        n_old = length(m.y)
        append!(m.ds, ds); append!(m.y, ys[j]); append!(m.perm, n_old+1:n_old+length(ds))
        lm = [(o.info[k] != 0 || !isfinite(o.logml_full[j, k])) ? -Inf : o.logml_full[j, k]
              for k in 1:length(m.particles)]
        m.log_weights = _advance(m.log_weights, lm, m.logml)
        m.logml = lm
        m.n_obs = length(m.y)
    end
    return ms
end

struct Mixture
    means::Matrix{Float64}      # m x P
    covs::Array{Float64, 3}     # m x m x P
    weights::Vector{Float64}
end
function Base.rand(rng::AbstractRNG, d::Mixture, k::Integer)
    m = size(d.means, 1); out = Matrix{Float64}(undef, m, k); cw = cumsum(d.weights)
    for j in 1:k
        c = min(searchsortedfirst(cw, rand(rng)), length(cw))
        out[:, j] = d.means[:, c] + cholesky(Symmetric(d.covs[:, :, c])).L * randn(rng, m)
    end
    return out
end
Base.rand(d::Mixture, k::Integer) = rand(Random.default_rng(), d, k)     # src/forecasting.jl:47
Base.rand(d::Mixture) = vec(rand(d, 1))                                  # src/forecasting.jl:67

const NGP_MAX_AUX = 192      # include/ngp.h: appended + forecast rows one call carries
"""
Forecast dates one library call carries beside n observations and d appended points
(include/ngp.h: (n mod 64) + d + m + 1 <= NGP_MAX_AUX).  The Python mirror serves longer horizons
by querying blocks of dates pairwise (nowcastautogp_amd/autogp.py `horizon_blocks`,
`predict_in_blocks`); this shim states the limit instead.
"""
horizon_room(n_obs::Int, d::Int = 0) = NGP_MAX_AUX - n_obs % 64 - d - 1
function _check_horizon(n_obs::Int, m::Int)
    m <= horizon_room(n_obs) || throw(ArgumentError(
        "predict_mvn: $m forecast dates, but one call carries at most $(horizon_room(n_obs)) beside " *
        "$n_obs observations (NGP_MAX_AUX = $NGP_MAX_AUX); query the dates in blocks"))
end

"AutoGP.predict_mvn(model, dates) — src/forecasting.jl:46, 66"
function predict_mvn(m::GPModel, dates::AbstractVector{<:Dates.TimeType})
    return predict_mvn_lockstep([m], dates)[1]
end
"D models on the same dates: ONE `ngp_predict_batch` call of P x D items."
function predict_mvn_lockstep(ms::Vector{GPModel}, dates::AbstractVector{<:Dates.TimeType})
    t, ys = _group_obs(ms)
    _check_horizon(length(t), length(dates))
    t_new = _model_time(ms[1], dates)
    progs = reduce(vcat, (m.particles for m in ms))
    owner = [j for (j, m) in enumerate(ms) for _ in m.particles]
    mu, sigma, _, info = predict_batch(ms[1].ctx, progs, t, _item_y(ys, owner), t_new)
    raise_if_not_posdef(info)
    w, _, _ = weights_normalize_cols(reduce(hcat, (m.log_weights for m in ms)))
    out = Mixture[]
    off = 0
    for (j, m) in enumerate(ms)
        r = off+1:off+length(m.particles)
        push!(out, Mixture((mu[:, r] .- m.y_intercept) ./ m.y_slope, sigma[:, :, r] ./ m.y_slope^2,
                           w[:, j]))
        off += length(m.particles)
    end
    return out
end

"One additive part of a particle's kernel: `kind` is :trend (a Linear inside), :seasonal (a Periodic and no Linear) or :other."
struct Component
    tree::Node
    label::String
    kind::Symbol
end
component_kind(p::Program) = 2 in p.ops ? :trend : (5 in p.ops ? :seasonal : :other)
const NODE_NAMES = ("Constant", "Linear", "SquaredExponential", "GammaExponential", "Periodic", "Plus",
                    "Times", "ChangePoint")
function label(n::Node)
    ps = join(string.(n.params), ", ")
    isleaf(n) && return "$(NODE_NAMES[n.op])($ps)"
    return "$(NODE_NAMES[n.op])($(label(n.left)), $(label(n.right))$(isempty(ps) ? "" : ", " * ps))"
end

"AutoGP.decompose: per particle the additive parts of its kernel (a ChangePoint is one part)."
function decompose(m::GPModel)
    return [[Component(from_program(c), label(from_program(c)), component_kind(c))
             for c in kernel_components(p)] for p in m.particles]
end

"""
The additive decomposition of the forecast on `dates`, original scale of y: per particle `means`
(m x C_p), `var` (m x C_p) and the joint `sigma` of its parts, the particle `weights`, the parts'
`kinds`, and `offset` — the constant of the y-transform, which belongs to no part (forecast without
noise = offset + sum of the parts).  One query of a resident factor (`ngp_factor_components`); the
horizon is limited as stated by `components` (the Python mirror serves longer ones in date blocks).
"""
function predict_components(m::GPModel, dates::AbstractVector{<:Dates.TimeType})
    parts = decompose(m)
    t, y = _obs(m)
    cmax = maximum(length.(parts))
    cmax * length(dates) <= horizon_room(length(t)) || throw(ArgumentError(
        "predict_components: $(length(dates)) dates x $cmax parts, but one call carries at most " *
        "$(horizon_room(length(t))) rows beside $(length(t)) observations (NGP_MAX_AUX = $NGP_MAX_AUX)"))
    f = Factor(m.ctx, m.particles, t, y)
    comps = [[Program(c.ops, c.params, 0.0) for c in kernel_components(p)] for p in m.particles]
    o = components(f, comps, _model_time(m, dates))
    raise_if_not_posdef(o.info)
    w, _, _ = weights_normalize(m.log_weights)
    s = 1 / m.y_slope
    return (means = [a .* s for a in o.mu], var = [a .* s^2 for a in o.var],
            sigma = [a .* s^2 for a in o.sigma], weights = w,
            kinds = [[c.kind for c in ps] for ps in parts], offset = -m.y_intercept * s)
end

"""
What `forecast_with_nowcasts` (src/forecasting.jl:117-167) does with its scenarios, as ONE ensemble
instead of one `Threads.@spawn` task per scenario: clone, `add_data!`, `maybe_resample!`, the
requested refinement, then the forecast draws — every step one library call of P x D items.  A
maintainer replaces the task fan-out (src/forecasting.jl:131-165) by a call of this function; the
result is the `hcat` of the per-scenario forecasts (m x (D * draws)), before `inv_transformation`.
"""
function forecast_with_nowcasts_lockstep(base::GPModel, nowcast_ds::AbstractVector{<:Dates.TimeType},
                                         nowcast_ys::Vector{<:AbstractVector{<:Real}},
                                         dates::AbstractVector{<:Dates.TimeType}, draws::Int;
                                         n_mcmc::Int = 0, n_hmc::Int = 0, ess_threshold::Real = 0.0,
                                         forecast_n_hmc::Union{Nothing, Int} = nothing,
                                         hmc_config = DEFAULT_HMC)
    snapshot = Dict(base)                                                   # src/forecasting.jl:128
    ms = [GPModel(deepcopy(snapshot); ctx = base.ctx, rng = Random.Xoshiro(rand(base.rng, UInt64)))
          for _ in nowcast_ys]                                              # :133, own stream each
    add_data_lockstep!(ms, nowcast_ds, nowcast_ys, base)                    # :135
    maybe_resample_lockstep!(ms, ess_threshold * num_particles(base))       # :138-141
    if n_mcmc > 0 && n_hmc > 0
        mcmc_structure_lockstep!(ms, n_mcmc, n_hmc; hmc_config)             # :146
    elseif n_hmc > 0
        mcmc_parameters_lockstep!(ms, n_hmc; hmc_config)                    # :148
    end
    m = length(dates)
    out = [Matrix{Float64}(undef, m, draws) for _ in ms]
    if forecast_n_hmc === nothing                                           # :39-52
        for (o, mix, mdl) in zip(out, predict_mvn_lockstep(ms, dates), ms)
            o .= rand(mdl.rng, mix, draws)
        end
    else                                                                    # :54-75
        for i in 1:draws
            mcmc_parameters_lockstep!(ms, forecast_n_hmc; hmc_config)
            for (o, mix, mdl) in zip(out, predict_mvn_lockstep(ms, dates), ms)
                o[:, i] = vec(rand(mdl.rng, mix, 1))
            end
        end
    end
    return reduce(hcat, out)
end

# ---- Dict(model) / GPModel(::Dict): the version-1 wire format of nowcastautogp_amd/wire.py
#      (src/forecasting.jl:128, 133; the dict is plain data, so deepcopy is a data copy) -------------
function Base.Dict(m::GPModel)
    sp = get_spec(m.ctx)
    cfg = m.config
    return Dict{String, Any}(
        "format" => "ngp-model", "version" => 1,
        "config" => Dict{String, Any}(
            "node_dist_leaf" => copy(cfg.node_dist_leaf), "node_dist_nocp" => copy(cfg.node_dist_nocp),
            "node_dist_cp" => copy(cfg.node_dist_cp), "max_branch" => cfg.max_branch,
            "max_depth" => cfg.max_depth, "changepoints" => cfg.changepoints, "noise" => cfg.noise,
            "prior" => Dict{String, Any}(String(k) => Dict{String, Any}("mu" => v[:mu], "sigma" => v[:sigma])
                                         for (k, v) in cfg.prior)),
        "spec" => Dict{String, Any}("se_form" => sp.se_form, "periodic_form" => sp.periodic_form,
                                    "cp_form" => sp.cp_form, "jitter" => sp.jitter),
        "data" => Dict{String, Any}("ds_kind" => "date", "ds" => [string(d) for d in m.ds],
                                    "y" => copy(m.y)),
        "transforms" => Dict{String, Any}(
            "ds" => Dict{String, Any}("slope" => m.ds_slope, "intercept" => m.ds_intercept),
            "y" => Dict{String, Any}("slope" => m.y_slope, "intercept" => m.y_intercept)),
        "n_obs" => m.n_obs, "perm" => m.perm .- 1,
        "n_particles_total" => length(m.particles), "particle_offset" => 0,
        "particles" => [Dict{String, Any}("ops" => Int.(p.ops), "params" => copy(p.params),
                                          "noise" => p.noise) for p in m.particles],
        "log_weights" => copy(m.log_weights), "logml" => copy(m.logml),
        "depth_cap" => m.depth_cap)
    # "rng" is optional in the format: Julia's stream is not portable, a reader reseeds
end

function GPModel(d::AbstractDict; ctx::Context = default_context(),
                 rng::AbstractRNG = Random.default_rng())
    d["format"] == "ngp-model" && d["version"] == 1 ||
        throw(ArgumentError("not a version-1 ngp-model dict"))
    c = d["config"]
    prior = Dict{Symbol, Dict{Symbol, Float64}}(
        Symbol(k) => Dict(:mu => Float64(v["mu"]), :sigma => Float64(v["sigma"])) for (k, v) in c["prior"])
    cfg = GPConfig(node_dist_leaf = Float64.(c["node_dist_leaf"]),
                   node_dist_nocp = Float64.(c["node_dist_nocp"]),
                   node_dist_cp = Float64.(c["node_dist_cp"]), max_branch = c["max_branch"],
                   max_depth = c["max_depth"], changepoints = c["changepoints"],
                   noise = c["noise"] === nothing ? nothing : Float64(c["noise"]), prior = prior)
    d["data"]["ds_kind"] == "date" || throw(ArgumentError("this reader needs date-valued ds"))
    # the cached per-particle logml belongs to the formula variants / jitter it was computed under
    # (nowcastautogp_amd/wire.py refuses the same mismatch)
    sp, ws = get_spec(ctx), d["spec"]
    (ws["se_form"] == sp.se_form && ws["periodic_form"] == sp.periodic_form &&
     ws["cp_form"] == sp.cp_form && ws["jitter"] == sp.jitter) ||
        throw(ArgumentError("ngp-model dict was written under another spec than this context runs"))
    parts = [Program(Int32.(p["ops"]), Float64.(p["params"]), Float64(p["noise"]))
             for p in d["particles"]]
    tr = d["transforms"]
    return GPModel(cfg, Date.(d["data"]["ds"]), Float64.(d["data"]["y"]), parts,
                   Float64.(d["log_weights"]), Float64.(d["logml"]), d["n_obs"],
                   Int.(d["perm"]) .+ 1, tr["ds"]["slope"], tr["ds"]["intercept"],
                   tr["y"]["slope"], tr["y"]["intercept"], d["depth_cap"], rng, ctx)
end

end # module
