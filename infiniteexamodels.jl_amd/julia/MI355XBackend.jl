# MI355XBackend.jl — the Julia side of the drop-in boundary (UNEXECUTED: there is no
# `julia` in the build image; written against include/iem.h and the reference's plug point).
#
# Usage in the reference (README.md:41 has `backend = CUDABackend()` in this slot):
#
#     using InfiniteOpt, InfiniteExaModels, MadNLP, AMDGPU
#     include("MI355XBackend.jl"); using .MI355X
#     model = InfiniteModel(ExaTranscriptionBackend(MadNLPSolver; backend = MI355XBackend()))
#
# `ExaTranscriptionBackend` stores the value untyped (`src/infiniteopt_backend.jl:100`) and
# forwards it to `ExaModels.ExaCore(...; backend)` (`src/transform.jl:815`); the two methods
# below intercept `ExaCore`/`ExaModel` construction for `MI355XBackend`, so the transcriber
# (`build_exa_core!`, `src/transform.jl:771-796`) runs unchanged on a host core and the
# finished core is handed to libiem_hip.so as a blob.
module MI355X

using ExaModels, NLPModels, AMDGPU

export MI355XBackend, MI355XModel

const LIBIEM = get(ENV, "LIBIEM_HIP", "libiem_hip.so")

struct MI355XBackend
    device::Int
end
MI355XBackend() = MI355XBackend(0)

struct IemError <: Exception
    code::Cint
    msg::String
end
function check(rc::Cint)
    rc == 0 && return
    throw(IemError(rc, unsafe_string(ccall((:iem_last_error, LIBIEM), Cstring, ()))))
end

# struct iem_meta_t (include/iem.h)
struct IemMeta
    nvar::Int64; ncon::Int64; npar::Int64; nnzj::Int64; nnzh::Int64; n_templates::Int64
    minimize::Int32; n_kernels::Int32
end

mutable struct MI355XModel <: NLPModels.AbstractNLPModel{Float64, ROCVector{Float64}}
    handle::Ptr{Cvoid}
    meta::NLPModels.NLPModelMeta{Float64, ROCVector{Float64}}
    counters::NLPModels.Counters
    θ::Vector{Float64}              # host mirror (infiniteopt_backend.jl:479 reads model.θ)
    core::Any                       # the host ExaCore the transcriber filled
end

host_array(h, which, n) = (out = Vector{Float64}(undef, n);
    check(ccall((:iem_get_host, LIBIEM), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), h, which, out)); out)

# ExaModels.ExaModel(core) at src/infiniteopt_backend.jl:156, for cores built with MI355XBackend
function MI355XModel(core, backend::MI355XBackend)
    blob = to_blob(core)                              # include/iem_blob.h
    href = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_create, LIBIEM), Cint, (Ptr{UInt8}, Csize_t, Cint, Ptr{Ptr{Cvoid}}),
                blob, length(blob), backend.device, href))
    h = href[]
    m = Ref{IemMeta}()
    check(ccall((:iem_meta, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMeta}), h, m))
    mt = m[]
    dev(v) = ROCVector{Float64}(v)
    meta = NLPModels.NLPModelMeta(mt.nvar;
        ncon = mt.ncon, nnzj = mt.nnzj, nnzh = mt.nnzh, minimize = mt.minimize != 0,
        x0 = dev(host_array(h, 0, mt.nvar)), lvar = dev(host_array(h, 1, mt.nvar)),
        uvar = dev(host_array(h, 2, mt.nvar)), lcon = dev(host_array(h, 3, mt.ncon)),
        ucon = dev(host_array(h, 4, mt.ncon)), y0 = dev(host_array(h, 5, mt.ncon)))
    model = MI355XModel(h, meta, NLPModels.Counters(), host_array(h, 6, mt.npar), core)
    finalizer(x -> ccall((:iem_destroy, LIBIEM), Cint, (Ptr{Cvoid},), x.handle), model)
    return model
end

dptr(v::ROCVector{Float64}) = Ptr{Float64}(UInt(pointer(v)))

# ---- NLPModels API: one ccall each ------------------------------------------------------
function NLPModels.obj(m::MI355XModel, x::ROCVector{Float64})
    out = Ref{Float64}()
    check(ccall((:iem_obj, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), out))
    return out[]
end
NLPModels.grad!(m::MI355XModel, x::ROCVector{Float64}, g::ROCVector{Float64}) =
    (check(ccall((:iem_grad, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(g))); g)
NLPModels.cons_nln!(m::MI355XModel, x::ROCVector{Float64}, c::ROCVector{Float64}) =
    (check(ccall((:iem_cons, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(c))); c)
NLPModels.jac_coord!(m::MI355XModel, x::ROCVector{Float64}, v::ROCVector{Float64}) =
    (check(ccall((:iem_jac_coord, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(v))); v)
function NLPModels.hess_coord!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64},
                               v::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_hess_coord, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(v)))
    return v
end
# jac_coord! + hess_coord! in ONE launch (include/iem.h: iem_jac_hess_coord) for a solver that evaluates both at an accepted
# point (MadNLP); identical bytes to the two calls above
function jac_hess_coord!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, jac::ROCVector{Float64},
                         hess::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_jac_hess_coord, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(jac), dptr(hess)))
    return jac, hess
end
# One launch per SOLVER PHASE (include/iem.h: iem_eval_trial / iem_eval_accepted / iem_eval_all; identical bytes to the separate
# calls): obj + cons! at a trial point of the line search, grad! + jac_coord! + hess_coord! at the accepted point
# (ext/InfiniteExaModelsMadNLP.jl:49-50,64).  `eval_trial!` returns f; with `defer = true` it returns at once and `obj_end`
# collects the value (a MadNLP callback that needs c first can overlap the scalar's round trip).
function eval_trial!(m::MI355XModel, x::ROCVector{Float64}, c::ROCVector{Float64}; defer = false)
    out = Ref{Float64}()
    check(ccall((:iem_eval_trial, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(c), defer ? C_NULL : out))
    return defer ? nothing : out[]
end
function eval_accepted!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, g::ROCVector{Float64}, jac::ROCVector{Float64},
                        hess::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_eval_accepted, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(g), dptr(jac), dptr(hess)))
    return g, jac, hess
end
function eval_all!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, c::ROCVector{Float64}, g::ROCVector{Float64},
                   jac::ROCVector{Float64}, hess::ROCVector{Float64}; obj_weight = 1.0)
    out = Ref{Float64}()
    check(ccall((:iem_eval_all, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(c), dptr(g), dptr(jac), dptr(hess), out))
    return out[]
end
# obj in two halves: obj_begin! first, obj_end after the last launch of the evaluation point — the scalar's host round trip
# overlaps grad!, cons!, jac_coord!, hess_coord! (ext/InfiniteExaModelsIpopt.jl:48-49 evaluates all five at one point)
obj_begin!(m::MI355XModel, x::ROCVector{Float64}) =
    (check(ccall((:iem_obj_begin, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}), m.handle, dptr(x))); m)
function obj_end(m::MI355XModel)
    out = Ref{Float64}()
    check(ccall((:iem_obj_end, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}), m.handle, out))
    return out[]
end
# sharded handles: the halo exchange off the critical path (it rides on the next evaluation launch that takes x and cannot
# touch a halo entry; include/iem.h: iem_halo_exchange_async)
halo_exchange_async!(m::MI355XModel, x::ROCVector{Float64}) =
    (check(ccall((:iem_halo_exchange_async, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}), m.handle, dptr(x))); x)
# optional set-up step, once the solver has allocated its COO value buffers: which of the handle's two code objects
# writes THESE buffers faster (include/iem.h: iem_tune); a no-op for handles with one code object
function tune!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, jac::ROCVector{Float64},
               hess::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_tune, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(jac), dptr(hess)))
    return m
end
function NLPModels.jac_structure!(m::MI355XModel, rows::AbstractVector{Int}, cols::AbstractVector{Int})
    r, c = Vector{Int64}(undef, m.meta.nnzj), Vector{Int64}(undef, m.meta.nnzj)
    check(ccall((:iem_jac_structure, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), m.handle, r, c, 1))
    copyto!(rows, r); copyto!(cols, c)
    return rows, cols
end
function NLPModels.hess_structure!(m::MI355XModel, rows::AbstractVector{Int}, cols::AbstractVector{Int})
    r, c = Vector{Int64}(undef, m.meta.nnzh), Vector{Int64}(undef, m.meta.nnzh)
    check(ccall((:iem_hess_structure, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), m.handle, r, c, 1))
    copyto!(rows, r); copyto!(cols, c)
    return rows, cols
end

NLPModels.jprod!(m::MI355XModel, x::ROCVector{Float64}, v::ROCVector{Float64}, Jv::ROCVector{Float64}) =
    (check(ccall((:iem_jprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(v), dptr(Jv))); Jv)
NLPModels.jtprod!(m::MI355XModel, x::ROCVector{Float64}, v::ROCVector{Float64}, Jtv::ROCVector{Float64}) =
    (check(ccall((:iem_jtprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(v), dptr(Jtv))); Jtv)
function NLPModels.hprod!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, v::ROCVector{Float64},
                          Hv::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_hprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), dptr(v), obj_weight, dptr(Hv)))
    return Hv
end

# Parameter sensitivities (no NLPModels counterpart; unexecuted like the rest of this shim): the products with ∂/∂θ at
# (x, the handle's current θ) — (∂c/∂θ)·w, obj_weight·∂f/∂θ + (∂c/∂θ)ᵀ·y, (∂²L/∂x∂θ)·w.  K·[dx; dy] = -[hpprod!; jpprod!] is
# the first-order move of a solution under δθ = w.
jpprod!(m::MI355XModel, x::ROCVector{Float64}, w::ROCVector{Float64}, out::ROCVector{Float64}) =
    (check(ccall((:iem_jpprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(w), dptr(out))); out)
function jptprod!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, out::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_jptprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(out)))
    return out
end
function hpprod!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, w::ROCVector{Float64},
                 out::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_hpprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(w), dptr(out)))
    return out
end
# ... and the transpose of hpprod!, (∂²L/∂θ∂x)·u (u over x, out over θ): with λ = K⁻¹·[∂q/∂x; ∂q/∂y] (K symmetric),
# dq/dθ = ∂q/∂θ - (hptprod!(x, y, λ_x) + jptprod!(x, λ_y; obj_weight = 0)) — every entry of θ from one solve.
function hptprod!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, u::ROCVector{Float64},
                  out::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_hptprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(u), dptr(out)))
    return out
end
# ... and the θθ block (∂²L/∂θ²)·w (w and out over θ; symmetric): with (dx, dy) the parameter step of δθ,
# φ''(θ)·δθ = hppprod!(x, y, δθ) + hptprod!(x, y, dx) + jptprod!(x, dy; obj_weight = 0) for the value function φ(θ) = L(x*(θ), y*(θ), θ).
function hppprod!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, w::ROCVector{Float64},
                  out::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_hppprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(w), dptr(out)))
    return out
end
# The convergence check of a solver: r = obj_weight·∇f(x) + J(x)ᵀ·y (the dual infeasibility of Ipopt / MadNLP is r minus the
# bound multipliers) from one atomic-free kernel, and with c(x) and f(x) — a device scalar, obj[1] — from one launch.
function lagrangian_prepare!(m::MI355XModel)
    n = Ref{Int32}(0)
    check(ccall((:iem_lagrad_prepare, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int32}), m.handle, n))
    return Int(n[])
end
function lagrangian_grad!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, out::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_lagrad, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(out)))
    return out
end
function eval_residual!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, c::ROCVector{Float64},
                        r::ROCVector{Float64}, obj::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_eval_residual, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(c), dptr(r), dptr(obj)))
    return obj, c, r
end
# Row scaling inside the kernels (Ipopt's gradient-based scaling, MadNLP's scale_constraints!): the row maxima of the Jacobian
# from one kernel — no triplet buffer —, and cons! / jac_coord! with every value times its row's factor s[row] in front of the
# store (bitwise c .* s and vals .* s[rows]).  The scaled Hessian is hess_coord!(m, x, y .* s, vals; obj_weight = σ * obj_scale).
function scaled_prepare!(m::MI355XModel)
    n = Ref{Int32}(0)
    check(ccall((:iem_scaled_prepare, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int32}), m.handle, n))
    return Int(n[])
end
function jac_row_maxabs!(m::MI355XModel, x::ROCVector{Float64}, out::ROCVector{Float64})
    check(ccall((:iem_jac_rowmax, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(out)))
    return out
end
function cons_scaled!(m::MI355XModel, x::ROCVector{Float64}, s::ROCVector{Float64}, c::ROCVector{Float64})
    check(ccall((:iem_cons_scaled, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(s), dptr(c)))
    return c
end
function jac_coord_scaled!(m::MI355XModel, x::ROCVector{Float64}, s::ROCVector{Float64}, vals::ROCVector{Float64})
    check(ccall((:iem_jac_coord_scaled, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(s), dptr(vals)))
    return vals
end
# One launch per solver phase for the scaled NLP (a ninth program of the handle): s the row factors, obj_scale the factor of the
# objective.  eval_trial_scaled! gives (obj_scale * f, s .* c), eval_accepted_scaled! gives obj_scale * ∇f, s[rows] .* jac and
# hess_coord!(x, y .* s; obj_weight * obj_scale) — bitwise the scaled calls above / the composed ones.  A model without
# constraints passes `nothing` for s, y, c and jac.
spptr(v) = v === nothing ? Ptr{Float64}(C_NULL) : dptr(v)
function scaled_phase_prepare!(m::MI355XModel)
    n = Ref{Int32}(0)
    check(ccall((:iem_scaled_phase_prepare, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int32}), m.handle, n))
    return Int(n[])
end
function grad_scaled!(m::MI355XModel, x::ROCVector{Float64}, obj_scale::Real, g::ROCVector{Float64})
    check(ccall((:iem_grad_scaled, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cdouble, Ptr{Float64}), m.handle, dptr(x), obj_scale, dptr(g)))
    return g
end
function hess_coord_scaled!(m::MI355XModel, x::ROCVector{Float64}, y, s, vals::ROCVector{Float64}; obj_weight = 1.0)
    check(ccall((:iem_hess_coord_scaled, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                m.handle, dptr(x), spptr(y), spptr(s), obj_weight, dptr(vals)))
    return vals
end
function eval_trial_scaled!(m::MI355XModel, x::ROCVector{Float64}, s, obj_scale::Real, c)
    f = Ref{Float64}(0.0)
    check(ccall((:iem_eval_trial_scaled, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), spptr(s), obj_scale, spptr(c), f))
    return f[], c
end
function eval_accepted_scaled!(m::MI355XModel, x::ROCVector{Float64}, y, s, obj_scale::Real, g::ROCVector{Float64}, jac,
                               hess; obj_weight = 1.0)
    check(ccall((:iem_eval_accepted_scaled, LIBIEM), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), spptr(y), spptr(s), obj_scale, obj_weight, dptr(g), spptr(jac), spptr(hess)))
    return g, jac, hess
end
# The KKT operator in one launch: out_x = W u + J' v, out_y = J u with W = obj_weight ∇²f + Σ y_r ∇²c_r — the product with
# [W J'; J 0] a matrix-free method (and the residual of a Newton step) needs.  v === nothing means v = 0; outputs may not alias inputs.
function kktprod_prepare!(m::MI355XModel)
    n = Ref{Int32}(0)
    check(ccall((:iem_kktprod_prepare, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int32}), m.handle, n))
    return Int(n[])
end
function kktprod!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, u::ROCVector{Float64}, v, out_x::ROCVector{Float64},
                  out_y::ROCVector{Float64}; obj_weight = 1.0)
    pv = v === nothing ? Ptr{Float64}(C_NULL) : dptr(v)
    check(ccall((:iem_kktprod, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, dptr(u), pv, dptr(out_x), dptr(out_y)))
    return out_x, out_y
end
# ... and the three blocks themselves in COO (include/iem.h has the slot order and the triangle convention of ∂²L/∂θ²):
# Jθ = ∂c/∂θ, Hxθ = ∂²L/∂x∂θ, Hθθ = ∂²L/∂θ² — what a host with its own linear algebra assembles G = [Hxθ; Jθ] from.
function param_coord_nnz(m::MI355XModel)
    out = zeros(Int64, 3)
    check(ccall((:iem_param_coord_nnz, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}), m.handle, out))
    return (out[1], out[2], out[3])
end
function param_coord_prepare!(m::MI355XModel)
    n = Ref{Int32}(0)
    check(ccall((:iem_param_coord_prepare, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int32}), m.handle, n))
    return Int(n[])
end
for (fn, sym, blk) in ((:jacp_structure!, :iem_jacp_structure, 1), (:hessxp_structure!, :iem_hessxp_structure, 2), (:hesspp_structure!, :iem_hesspp_structure, 3))
    @eval function $fn(m::MI355XModel, rows::Vector{Int64}, cols::Vector{Int64})      # 1-based, like jac_structure!
        @assert length(rows) == length(cols) == param_coord_nnz(m)[$blk]
        check(ccall(($(QuoteNode(sym)), LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), m.handle, rows, cols, 1))
        return rows, cols
    end
end
function jacp_coord!(m::MI355XModel, x::ROCVector{Float64}, vals::ROCVector{Float64})
    check(ccall((:iem_jacp_coord, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(x), dptr(vals)))
    return vals
end
# both second-order blocks from one launch; pass `nothing` for a block that is not wanted (not for both)
function hessp_coord!(m::MI355XModel, x::ROCVector{Float64}, y::ROCVector{Float64}, hessxp, hesspp; obj_weight = 1.0)
    px = hessxp === nothing ? Ptr{Float64}(C_NULL) : dptr(hessxp)
    pp = hesspp === nothing ? Ptr{Float64}(C_NULL) : dptr(hesspp)
    check(ccall((:iem_hessp_coord, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
                m.handle, dptr(x), dptr(y), obj_weight, px, pp))
    return hessxp, hesspp
end

# ExaModels.set_parameter!(core, param, vals)  (src/infiniteopt_backend.jl:522,546)
function set_parameter!(m::MI355XModel, param, vals)
    v = collect(Float64, vec(vals))
    m.θ[param.offset+1:param.offset+param.length] .= v
    check(ccall((:iem_set_parameter, LIBIEM), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}),
                m.handle, param.offset, length(v), v))
end

# ---- multi-GPU: one process per GPU (e.g. under MPI.jl) ----------------------------------------
# UNEXECUTED, like the rest of this file.  Every rank builds the SAME global core; the library cuts the
# rank's support window (include/iem.h: iem_create_sharded) — `slabs` / `template_groups` as for to_blob.
# `allgather(bytes) -> Vector{UInt8}` is the host's transport (MPI.Allgather, ...): 128 bytes per rank.
function MI355XShardedModel(core, backend::MI355XBackend, group::Int, rank::Int, world::Int, allgather;
                            slabs, template_groups = nothing)
    blob = to_blob(core; slabs = slabs, template_groups = template_groups)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_create_sharded, LIBIEM), Cint,
                (Ptr{UInt8}, Csize_t, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}),
                blob, length(blob), backend.device, group, rank, world, C_NULL, 0, h))
    mine = Vector{UInt8}(undef, 128)                       # IEM_COMM_HANDLE_BYTES
    check(ccall((:iem_comm_export, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{UInt8}), h[], mine))
    check(ccall((:iem_comm_connect, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{UInt8}), h[], allgather(mine)))
    return h[]                                             # wrap like MI355XModel(core, backend) (meta from iem_meta)
end
# both directions of the halo: (halo_left, halo_right, reach_left, reach_right, doubles_to_right, doubles_to_left); a model with
# forward / central differences (transform.jl:535: any finite-difference method) has reach_right > 0 and exchanges both ways
function shard_halo(m::MI355XModel)
    out = Vector{Int64}(undef, 6)
    check(ccall((:iem_shard_halo, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}), m.handle, out))
    return (halo_left = out[1], halo_right = out[2], reach_left = out[3], reach_right = out[4], doubles_to_right = out[5], doubles_to_left = out[6])
end
# before cons!/jac_coord!/hess_coord!: the stencil neighbours x_k[a_r - 1] from the left rank (transform.jl:535-557)
halo_exchange!(m::MI355XModel, x::ROCVector{Float64}) =
    (check(ccall((:iem_halo_exchange, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}), m.handle, dptr(x))); x)
# after jtprod! on this rank's rows: the transposed exchange (halo-copy entries -> the left rank's owned entries), then
# allreduce_obj_grad! for the entries of replicated variables
halo_fold!(m::MI355XModel, v::ROCVector{Float64}) =
    (check(ccall((:iem_halo_fold, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}), m.handle, dptr(v))); v)
# after obj (device scalar f) / grad!: objective + gradient entries of replicated variables, summed over the ranks
allreduce_obj_grad!(m::MI355XModel, f::ROCVector{Float64}, g::ROCVector{Float64}) =
    (check(ccall((:iem_allreduce_obj_grad, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, dptr(f), dptr(g))); (f, g))

# ---- the linear solver behind MadNLP's AbstractLinearSolver slot (where README.md:36-37 picks CUDSSSolver) ----------
# UNEXECUTED, like the rest of this file; [EXT]: MadNLP's linear-solver interface (factorize!, solve!, is_inertia, inertia)
# from memory of MadNLP 0.8.  One object holds the analysis (grouping by support, coupling rows / columns, gather plan from
# the hess_coord! / jac_coord! value buffers) and the device blocks: include/iem.h, iem_kkt_*.  `hess`, `jac`, `sigma` are the
# solver's own value buffers (MadNLP's sparse KKT system keeps them); delta_w / delta_c its current regularisation.
mutable struct ChainKKTSolver <: Any      # <: MadNLP.AbstractLinearSolver{Float64} once MadNLP is loaded next to this file
    k::Ptr{Cvoid}
    hess::ROCVector{Float64}; jac::ROCVector{Float64}; sigma::ROCVector{Float64}
    delta_w::Float64; delta_c::Float64
    inertia::Vector{Int64}
end
function ChainKKTSolver(m::MI355XModel, hess, jac, sigma)
    k = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_kkt_create, LIBIEM), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}), m.handle, 0, k))   # refuses what it cannot hold
    s = ChainKKTSolver(k[], hess, jac, sigma, 0.0, 0.0, zeros(Int64, 3))
    finalizer(s -> ccall((:iem_kkt_destroy, LIBIEM), Cint, (Ptr{Cvoid},), s.k), s)      # before the model's own finalizer
    return s
end
function factorize!(s::ChainKKTSolver)
    check(ccall((:iem_kkt_assemble, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                s.k, dptr(s.hess), dptr(s.jac), dptr(s.sigma), s.delta_w, s.delta_c))
    check(ccall((:iem_kkt_factor, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.k, s.inertia))
    return s
end
solve!(s::ChainKKTSolver, x::ROCVector{Float64}) =       # in place: the right-hand side is read before the solution is written
    (check(ccall((:iem_kkt_solve, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.k, dptr(x), dptr(x))); x)
solve!(s::ChainKKTSolver, X::ROCMatrix{Float64}) =       # the columns of X in one pass over the factors (iem_kkt_solve_many), in place
    (check(ccall((:iem_kkt_solve_many, LIBIEM), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64), s.k, size(X, 2), dptr(X), stride(X, 2), dptr(X), stride(X, 2))); X)
# r = rhs − K sol at (x, y, obj_weight) with the solver's own sigma / delta_w / delta_c, matrix-free (iem_kkt_residual); `norm`: a
# device vector of one entry that receives max |r|, or nothing
function residual!(s::ChainKKTSolver, x::ROCVector{Float64}, y::ROCVector{Float64}, rhs::ROCVector{Float64}, sol::ROCVector{Float64},
                   r::ROCVector{Float64}; obj_weight = 1.0, norm = nothing)
    pn = norm === nothing ? Ptr{Float64}(C_NULL) : dptr(norm)
    check(ccall((:iem_kkt_residual, LIBIEM), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                s.k, dptr(x), dptr(y), obj_weight, dptr(s.sigma), s.delta_w, s.delta_c, dptr(rhs), dptr(sol), dptr(r), pn))
    return r
end
# sol = solve(rhs) and `steps` steps of iterative refinement against that residual, in one asynchronous call
# (iem_kkt_solve_refined); `norms`: a device vector of steps + 1 entries (max |r| in front of every step and behind the last), or nothing
function solve_refined!(s::ChainKKTSolver, x::ROCVector{Float64}, y::ROCVector{Float64}, rhs::ROCVector{Float64}, sol::ROCVector{Float64};
                        obj_weight = 1.0, steps = 1, norms = nothing)
    pn = norms === nothing ? Ptr{Float64}(C_NULL) : dptr(norms)
    check(ccall((:iem_kkt_solve_refined, LIBIEM), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}),
                s.k, dptr(x), dptr(y), obj_weight, dptr(s.sigma), s.delta_w, s.delta_c, dptr(rhs), dptr(sol), steps, pn))
    return sol
end
# A PER-ROW diagonal in the constraint block (an interior-point method with eliminated slacks: Σs⁻¹ on the inequality rows):
# K = [W + Σ + δw·I, Jᵀ; J, −diag(dcon + δc)], `dcon` a device vector of ncon entries (nothing: zeros — iem_kkt_assemble itself).
# The entries are not inspected.  UNEXECUTED, like the rest of this file.
dcon_ptr(dcon) = dcon === nothing ? Ptr{Float64}(C_NULL) : dptr(dcon)
function factorize_diag!(s::ChainKKTSolver, dcon)
    check(ccall((:iem_kkt_assemble_diag, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                s.k, dptr(s.hess), dptr(s.jac), dptr(s.sigma), dcon_ptr(dcon), s.delta_w, s.delta_c))
    check(ccall((:iem_kkt_factor, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.k, s.inertia))
    return s
end
# R = RHS − K·SOL column for column (iem_kkt_residual_diag: one operator launch per column, one finishing launch per eight);
# `norms`: a device vector of size(RHS, 2) entries that receives max |r| per column, or nothing.  R may be RHS itself.
function residual_diag!(s::ChainKKTSolver, x::ROCVector{Float64}, y::ROCVector{Float64}, dcon, RHS::ROCMatrix{Float64}, SOL::ROCMatrix{Float64},
                        R::ROCMatrix{Float64}; obj_weight = 1.0, norms = nothing)
    pn = norms === nothing ? Ptr{Float64}(C_NULL) : dptr(norms)
    check(ccall((:iem_kkt_residual_diag, LIBIEM), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                 Ptr{Float64}, Int64, Ptr{Float64}),
                s.k, dptr(x), dptr(y), obj_weight, dptr(s.sigma), dcon_ptr(dcon), s.delta_w, s.delta_c, size(RHS, 2), dptr(RHS), stride(RHS, 2),
                dptr(SOL), stride(SOL, 2), dptr(R), stride(R, 2), pn))
    return R
end
# SOL = K⁻¹ RHS with `steps` steps of refinement per column (iem_kkt_solve_refined_diag: iem_kkt_solve_many, then residuals, solves
# and one add per step); `norms`: a device matrix size(RHS, 2) x (steps + 1) — column i the norms in front of step i — or nothing
function solve_refined_diag!(s::ChainKKTSolver, x::ROCVector{Float64}, y::ROCVector{Float64}, dcon, RHS::ROCMatrix{Float64}, SOL::ROCMatrix{Float64};
                             obj_weight = 1.0, steps = 1, norms = nothing)
    pn = norms === nothing ? Ptr{Float64}(C_NULL) : dptr(norms)
    check(ccall((:iem_kkt_solve_refined_diag, LIBIEM), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                 Cint, Ptr{Float64}),
                s.k, dptr(x), dptr(y), obj_weight, dptr(s.sigma), dcon_ptr(dcon), s.delta_w, s.delta_c, size(RHS, 2), dptr(RHS), stride(RHS, 2),
                dptr(SOL), stride(SOL, 2), steps, pn))
    return SOL
end
# A dense border (first-stage variables, u(t) of a laned grid) on the device: mode 1 factorises its Schur complement with a
# Bunch–Kaufman LDL' in one workgroup and solves it there — solve! / solve_refined! then contain no synchronisation and can be
# captured; mode 0 (the default) keeps it on the host.  A no-op for models without a dense border.
border_on_device!(s::ChainKKTSolver, on::Bool = true) =
    (check(ccall((:iem_kkt_set_border, LIBIEM), Cint, (Ptr{Cvoid}, Cint), s.k, on ? 1 : 0)); s)
# factorize! without the read-back: (positive, negative, doubtful) into a device vector of three Int64 (mode 1, or no border)
function factorize_async!(s::ChainKKTSolver, inertia::ROCVector{Int64})
    check(ccall((:iem_kkt_assemble, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                s.k, dptr(s.hess), dptr(s.jac), dptr(s.sigma), s.delta_w, s.delta_c))
    check(ccall((:iem_kkt_factor_async, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.k, dptr(inertia)))
    return s
end
# the low-level pair on raw buffers (include/iem.h): Gs = G − Σ Gp[k] → F, piv (+ the pivot counters), xB = Gs⁻¹ (rB − Σ rBp[k])
border_factor!(m::MI355XModel, S, ne, n_border, G, Gp, F, piv::ROCVector{Int32}, info::ROCVector{Int64}; rel = 1e-14) =
    check(ccall((:iem_kkt_border_factor, LIBIEM), Cint,
                (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}, Cdouble),
                m.handle, S, ne, n_border, dptr(G), dptr(Gp), dptr(F), dptr(piv), dptr(info), rel))
border_solve!(m::MI355XModel, S, ne, n_border, nrhs, F, piv::ROCVector{Int32}, rBp, rB, xB) =
    check(ccall((:iem_kkt_border_solve, LIBIEM), Cint,
                (Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                m.handle, S, ne, n_border, nrhs, dptr(F), dptr(piv), dptr(rBp), dptr(rB), dptr(xB)))
is_inertia(::ChainKKTSolver) = true
inertia(s::ChainKKTSolver) = (s.inertia[1], s.inertia[3], s.inertia[2])      # (positive, zero, negative)

# ---- the interior-point barrier layer (include/iem.h: iem_barrier_*) --------------------------------------------------------
# What MadNLP's set_aug_diagonal! / set_aug_rhs! / get_alpha_max / finish_aug_solve! and Ipopt's PDSystemSolver right-hand side and
# IpoptCalculatedQuantities error terms compute between the evaluation calls and the linear solver, one launch each and every
# scalar on the device.  Vectors are full length (s, vL, vU, ds, dvL, dvU have ncon entries; those on equality rows are never
# touched).  A state is the tuple (x, s, y, zL, zU, vL, vU), directions are (ds, dzL, dzU, dvL, dvU).  UNEXECUTED, like the rest.
struct IemBarrierInfo      # iem_barrier_info_t
    struct_size::UInt64
    nvar::Int64; ncon::Int64; n_eq::Int64; n_ineq::Int64; n_xl::Int64; n_xu::Int64; n_sl::Int64; n_su::Int64; nz::Int64; workgroups::Int64
end
mutable struct BarrierLayer
    b::Ptr{Cvoid}
    info::IemBarrierInfo
end
hptr(v) = v === nothing ? Ptr{Float64}(C_NULL) : pointer(v)
# bounds: host vectors, or nothing for the handle's own (a scaled solver passes its scaled lcon / ucon)
function BarrierLayer(m::MI355XModel; relax = 1e-8, lvar = nothing, uvar = nothing, lcon = nothing, ucon = nothing)
    b = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_barrier_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Ptr{Cvoid}}),
                m.handle, hptr(lvar), hptr(uvar), hptr(lcon), hptr(ucon), relax, b))
    info = Ref(IemBarrierInfo(sizeof(IemBarrierInfo), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    check(ccall((:iem_barrier_info, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemBarrierInfo}), b[], info))
    layer = BarrierLayer(b[], info[])
    finalizer(l -> (l.b == C_NULL || ccall((:iem_barrier_destroy, LIBIEM), Cint, (Ptr{Cvoid},), l.b); l.b = C_NULL), layer)
    return layer
end
# x is projected in place; s, zL, zU, vL, vU are written
function barrier_start!(l::BarrierLayer, x, c, s, zL, zU, vL, vU; bound_push = 1e-2, bound_frac = 1e-2)
    check(ccall((:iem_barrier_start, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                l.b, dptr(x), spptr(c), spptr(s), dptr(zL), dptr(zU), spptr(vL), spptr(vU), bound_push, bound_frac))
    return x, s, zL, zU, vL, vU
end
# sigma, dcon, rhs: the inputs of factorize_diag! / solve_refined_diag!
function barrier_terms!(l::BarrierLayer, state, r, c, mu, sigma, dcon, rhs)
    check(ccall((:iem_barrier_terms, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                l.b, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(r), spptr(c), mu, dptr(sigma), spptr(dcon), dptr(rhs)))
    return sigma, dcon, rhs
end
# the directions from sol = [dx; dy] and alpha = (alpha_primal, alpha_dual) on the device; +0.0: the state or direction was unusable
function barrier_step!(l::BarrierLayer, state, sol, mu, tau, dirs, alpha)
    check(ccall((:iem_barrier_step, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                l.b, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(sol), mu, tau, spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5]), dptr(alpha)))
    return dirs, alpha
end
function barrier_update!(l::BarrierLayer, state, sol, dirs, alpha, mu; kappa_sigma = 1e10)
    check(ccall((:iem_barrier_update, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                l.b, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(sol), spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5]), dptr(alpha), mu, kappa_sigma))
    return state
end
# out: eight doubles on the device (include/iem.h lists them); r === nothing: out[1] is NaN
function barrier_error!(l::BarrierLayer, state, r, c, mu, out)
    check(ccall((:iem_barrier_error, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                l.b, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), spptr(r), spptr(c), mu, dptr(out)))
    return out
end
# out = (theta, sum log gap) at a trial (x, s, c): the bits barrier_error! writes to out[7], out[8]
function barrier_merit!(l::BarrierLayer, x, s, c, out)
    check(ccall((:iem_barrier_merit, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), l.b, dptr(x), spptr(s), spptr(c), dptr(out)))
    return out
end

# ---- the filter line search (include/iem.h: iem_search_*) ---------------------------------------------------------------------
# The decision of the iteration on the device: the slope of the barrier objective and the control block (search_begin!), the trial point
# (search_trial!), the acceptance test of Waechter and Biegler 2006, Algorithm A, with its filter (search_accept!).  One launch each, no
# read-back but search_state.  A ladder of K rungs (search_trial!, obj, cons, barrier_merit!, search_accept!) needs no host decision:
# alpha[1] ends as the accepted step length or +0.0, for which barrier_update! moves nothing.  UNEXECUTED, like the rest.
struct IemSearchOpts       # iem_search_opts_t
    struct_size::UInt64
    gamma_theta::Float64; gamma_phi::Float64; eta_phi::Float64; delta::Float64; s_theta::Float64; s_phi::Float64; alpha_floor::Float64
    max_trials::Int64; filter_capacity::Int64
end
struct IemSearchState      # iem_search_state_t: words 0-12 of the control block
    struct_size::UInt64
    alpha::Float64; alpha_max::Float64; phi0::Float64; theta0::Float64; slope::Float64; theta_min::Float64; theta_max::Float64; phi_trial::Float64; theta_trial::Float64
    status::Int64; trials::Int64; filter_count::Int64; flags::Int64      # status: 0 searching, 1 accepted f-type, 2 accepted h-type, 3 failed, 4 unusable
end
mutable struct FilterSearch
    s::Ptr{Cvoid}
    layer::BarrierLayer      # borrowed: kept alive
end
function FilterSearch(l::BarrierLayer; gamma_theta = 1e-5, gamma_phi = 1e-8, eta_phi = 1e-8, delta = 1.0, s_theta = 1.1, s_phi = 2.3, alpha_floor = 1e-16,
                      max_trials = 30, filter_capacity = 64)
    opts = Ref(IemSearchOpts(sizeof(IemSearchOpts), gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, alpha_floor, max_trials, filter_capacity))
    s = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_search_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemSearchOpts}, Ptr{Ptr{Cvoid}}), l.b, opts, s))
    fs = FilterSearch(s[], l)
    finalizer(f -> (f.s == C_NULL || ccall((:iem_search_destroy, LIBIEM), Cint, (Ptr{Cvoid},), f.s); f.s = C_NULL), fs)
    return fs
end
# a new barrier problem (mu changed): the filter emptied, the flags cleared
search_reset!(f::FilterSearch) = check(ccall((:iem_search_reset, LIBIEM), Cint, (Ptr{Cvoid},), f.s))
# obj: one double on the device (f), err: the eight of barrier_error! at this point, alpha: the two of barrier_step!
function search_begin!(f::FilterSearch, state, grad, sol, ds, obj, err, alpha, mu; obj_weight = 1.0)
    check(ccall((:iem_search_begin, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                f.s, spptr(state[1]), spptr(state[2]), spptr(grad), dptr(sol), spptr(ds), dptr(obj), dptr(err), dptr(alpha), mu, obj_weight))
end
function search_trial!(f::FilterSearch, state, sol, ds, xt, st)
    check(ccall((:iem_search_trial, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                f.s, spptr(state[1]), spptr(state[2]), dptr(sol), spptr(ds), spptr(xt), spptr(st)))
    return xt, st
end
# ft: one double on the device (f at the trial point), merit: the two of barrier_merit! there; alpha[1] becomes the accepted step length or +0.0
function search_accept!(f::FilterSearch, ft, merit, mu, alpha; obj_weight = 1.0)
    check(ccall((:iem_search_accept, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}), f.s, dptr(ft), dptr(merit), mu, obj_weight, dptr(alpha)))
    return alpha
end
# the one read-back (synchronises the stream)
function search_state(f::FilterSearch)
    st = Ref(IemSearchState(sizeof(IemSearchState), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    check(ccall((:iem_search_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemSearchState}), f.s, st))
    return st[]
end
# (control block: 16 words of 8 bytes, filter: filter_capacity pairs (theta, phi)) as device addresses
function search_device(f::FilterSearch)
    ctl, flt = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_search_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Float64}}), f.s, ctl, flt))
    return ctl[], flt[]
end

# ---- the second-order correction of the search (include/iem.h: iem_soc_*) -------------------------------------------------------------
# Between the first rejected trial and the first halving of alpha (Ipopt's TrySecondOrderCorrection): soc_open! behind the first rung, then
# per round soc_rhs!, solve_refined! (one column: rhs_soc -> sol_soc), barrier_step! on sol_soc, soc_trial!, obj, cons, barrier_merit!,
# soc_accept!; soc_select! copies an accepted correction over the first-order direction.  Every call is one launch, gated on the device
# by words 13-15 of the search's control block: a call that does not apply stores nothing.  UNEXECUTED, like the rest.
struct IemSocOpts          # iem_soc_opts_t
    struct_size::UInt64
    max_soc::Int64
    kappa_soc::Float64
end
struct IemSocState         # iem_soc_state_t: the status word, then words 13-15 of the control block
    struct_size::UInt64
    status::Int64
    state::Int64; rounds::Int64      # state: 0 none, 1 active, 2 accepted, 3 closed
    alpha_prev::Float64
end
mutable struct SecondOrderCorrection
    q::Ptr{Cvoid}
    search::FilterSearch      # borrowed: kept alive
end
function SecondOrderCorrection(f::FilterSearch; max_soc = 4, kappa_soc = 0.99)
    opts = Ref(IemSocOpts(sizeof(IemSocOpts), max_soc, kappa_soc))
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_soc_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemSocOpts}, Ptr{Ptr{Cvoid}}), f.s, opts, q))
    soc = SecondOrderCorrection(q[], f)
    finalizer(c -> (c.q == C_NULL || ccall((:iem_soc_destroy, LIBIEM), Cint, (Ptr{Cvoid},), c.q); c.q = C_NULL), soc)
    return soc
end
soc_open!(c::SecondOrderCorrection) = check(ccall((:iem_soc_open, LIBIEM), Cint, (Ptr{Cvoid},), c.q))
# cons: c at the current point, ct / st: at the latest trial point, rhs: of barrier_terms!
function soc_rhs!(c::SecondOrderCorrection, state, cons, ct, st, rhs, mu, rhs_soc)
    check(ccall((:iem_soc_rhs, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
                c.q, spptr(state[2]), spptr(state[3]), spptr(state[6]), spptr(state[7]), spptr(cons), spptr(ct), spptr(st), dptr(rhs), mu, dptr(rhs_soc)))
    return rhs_soc
end
function soc_trial!(c::SecondOrderCorrection, state, sol_soc, ds_soc, alpha_soc, xt, st)
    check(ccall((:iem_soc_trial, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                c.q, spptr(state[1]), spptr(state[2]), dptr(sol_soc), spptr(ds_soc), dptr(alpha_soc), spptr(xt), spptr(st)))
    return xt, st
end
# accepted: alpha takes both step lengths of alpha_soc; rejected: alpha and the search's status, trials and step length stay
function soc_accept!(c::SecondOrderCorrection, ft, merit, alpha_soc, mu, alpha; obj_weight = 1.0)
    check(ccall((:iem_soc_accept, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}),
                c.q, dptr(ft), dptr(merit), dptr(alpha_soc), mu, obj_weight, dptr(alpha)))
    return alpha
end
# dirs = (ds, dzL, dzU, dvL, dvU)
function soc_select!(c::SecondOrderCorrection, sol_soc, dirs_soc, sol, dirs)
    check(ccall((:iem_soc_select, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 12)...),
                c.q, dptr(sol_soc), spptr(dirs_soc[1]), spptr(dirs_soc[2]), spptr(dirs_soc[3]), spptr(dirs_soc[4]), spptr(dirs_soc[5]),
                dptr(sol), spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5])))
    return sol, dirs
end
# the one read-back (synchronises the stream)
function soc_state(c::SecondOrderCorrection)
    st = Ref(IemSocState(sizeof(IemSocState), 0, 0, 0, 0))
    check(ccall((:iem_soc_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemSocState}), c.q, st))
    return st[]
end
# the accumulated residual csoc (ncon doubles) as a device address
function soc_device(c::SecondOrderCorrection)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_soc_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), c.q, p))
    return p[]
end

# ---- the barrier parameter (include/iem.h: iem_mu_*) ---------------------------------------------------------------------------------
# mu, tau and the stopping test in a block of sixteen words on the device beside the BarrierLayer: mu_error! (twelve words: the eight of
# barrier_error! at mu = 0 bit for bit, then the minimum, the sum and the count of unusable values of the products gap·z) and mu_update!
# (the stopping test and the monotone rule; a search given to it has its filter emptied iff mu moved).  bind_mu! makes the kernels of a
# BarrierLayer, FilterSearch or SecondOrderCorrection read mu (and tau) from the block: their mu / tau arguments are then ignored and one
# captured iteration serves every barrier problem.  bind_mu!(obj, nothing) unbinds; unbind before the parameter is finalized.  The inner
# search of a Restoration keeps the restoration problem's own mu: never bind it.  UNEXECUTED, like the rest.
struct IemMuOpts           # iem_mu_opts_t
    struct_size::UInt64
    mu_init::Float64; kappa_eps::Float64; kappa_mu::Float64; tau_min::Float64; tol::Float64; mu_floor::Float64; s_max::Float64
end
struct IemMuState          # iem_mu_state_t: words 0-11 of the block
    struct_size::UInt64
    mu::Float64; tau::Float64; zeta::Float64; e0::Float64; e_mu::Float64; e_d::Float64; e_p::Float64; e_c0::Float64
    status::Int64; flags::Int64; decreases::Int64; updates::Int64      # status: 0 iterating, 1 converged, 2 unusable; flags bit 0: mu changed in the last update
end
mutable struct BarrierParameter
    p::Ptr{Cvoid}
    layer::BarrierLayer      # borrowed: kept alive
end
# mu_floor = 0: max(1e-11, tol/10)
function BarrierParameter(l::BarrierLayer; mu_init = 0.1, kappa_eps = 10.0, kappa_mu = 0.2, tau_min = 0.99, tol = 1e-8, mu_floor = 0.0, s_max = 100.0)
    opts = Ref(IemMuOpts(sizeof(IemMuOpts), mu_init, kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max))
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_mu_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMuOpts}, Ptr{Ptr{Cvoid}}), l.b, opts, p))
    par = BarrierParameter(p[], l)
    finalizer(q -> (q.p == C_NULL || ccall((:iem_mu_destroy, LIBIEM), Cint, (Ptr{Cvoid},), q.p); q.p = C_NULL), par)
    return par
end
# a new solve: mu = mu0, tau and sqrt(mu) from it, status iterating, flags and counters zero (asynchronous)
mu_reset!(q::BarrierParameter, mu0) = check(ccall((:iem_mu_reset, LIBIEM), Cint, (Ptr{Cvoid}, Cdouble), q.p, mu0))
# out: twelve doubles on the device; r is required
function mu_error!(q::BarrierParameter, state, r, c, out)
    check(ccall((:iem_mu_error, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 10)...),
                q.p, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(r), spptr(c), dptr(out)))
    return out
end
# out12: the twelve of mu_error!; search: a FilterSearch on the same BarrierLayer, or nothing
function mu_update!(q::BarrierParameter, out12; search = nothing)
    check(ccall((:iem_mu_update, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}), q.p, dptr(out12), search === nothing ? C_NULL : search.s))
end
# the one read-back (synchronises the stream)
function mu_state(q::BarrierParameter)
    st = Ref(IemMuState(sizeof(IemMuState), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    check(ccall((:iem_mu_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMuState}), q.p, st))
    return st[]
end
# the block (16 words of 8 bytes) as a device address
function mu_device(q::BarrierParameter)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_mu_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), q.p, p))
    return p[]
end
_mu_handle(q) = q === nothing ? C_NULL : q.p
bind_mu!(l::BarrierLayer, q) = check(ccall((:iem_barrier_bind_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), l.b, _mu_handle(q)))
bind_mu!(f::FilterSearch, q) = check(ccall((:iem_search_bind_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), f.s, _mu_handle(q)))
bind_mu!(c::SecondOrderCorrection, q) = check(ccall((:iem_soc_bind_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.q, _mu_handle(q)))

# ---- the adaptive barrier parameter (include/iem.h: iem_amu_*) -----------------------------------------------------------------------
# Ipopt's mu_strategy = adaptive (kkt-error globalisation; probing or LOQO oracle) ON a BarrierParameter, whose block it drives: the objects
# bound to that parameter follow.  Per iteration, in the place of mu_update!: mu_error!; amu_affine(amu, layer, search) do ... end around
# barrier_terms!(mu = 0), the back-solve of its rhs on the iteration's factors, barrier_step!(mu = 0, tau = 1) and amu_probe! (four words);
# amu_update!(amu, out12, probe4; search); amu_state — the one read-back, both blocks.  LOQO needs no affine solve: amu_update!(amu, out12,
# nothing).  Finalize (or let go of) the adaptive object before its BarrierParameter.  UNEXECUTED, like the rest.
struct IemAmuOpts          # iem_amu_opts_t
    struct_size::UInt64
    oracle::Int64          # 0 probing, 1 LOQO
    sigma_max::Float64; mu_min::Float64; mu_max_fact::Float64; init_factor::Float64; red_fact::Float64
    refs_max::Int64        # 1..4
end
struct IemAmuState         # iem_amu_state_t: words 0-13 of the object's own block
    struct_size::UInt64
    mode::Int64            # 0 free, 1 fixed
    mu_max::Float64
    refs_count::Int64
    refs::NTuple{4, Float64}      # oldest first
    mu_oracle::Float64; sigma::Float64; avg::Float64; m_aff::Float64
    to_fixed::Int64; to_free::Int64; oracle::Int64
end
mutable struct AdaptiveBarrierParameter
    a::Ptr{Cvoid}
    par::BarrierParameter      # borrowed: kept alive
end
function AdaptiveBarrierParameter(q::BarrierParameter; oracle = 0, sigma_max = 100.0, mu_min = 1e-11, mu_max_fact = 1e3, init_factor = 0.8, red_fact = 0.9999, refs_max = 4)
    opts = Ref(IemAmuOpts(sizeof(IemAmuOpts), oracle, sigma_max, mu_min, mu_max_fact, init_factor, red_fact, refs_max))
    a = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_amu_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemAmuOpts}, Ptr{Ptr{Cvoid}}), q.p, opts, a))
    amu = AdaptiveBarrierParameter(a[], q)
    finalizer(o -> (o.a == C_NULL || o.par.p == C_NULL || ccall((:iem_amu_destroy, LIBIEM), Cint, (Ptr{Cvoid},), o.a); o.a = C_NULL), amu)
    return amu
end
# a new solve: mode free, the ring empty, mu_max unset, counters zero (asynchronous); mu_reset! on the parameter is a call of its own
amu_reset!(o::AdaptiveBarrierParameter) = check(ccall((:iem_amu_reset, LIBIEM), Cint, (Ptr{Cvoid},), o.a))
# out: four doubles on the device; sol = [dx; dy] and dirs = (ds, dzL, dzU, dvL, dvU) of the affine step, alpha its two step lengths on the device
function amu_probe!(o::AdaptiveBarrierParameter, state, sol, dirs, alpha, out)
    check(ccall((:iem_amu_probe, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 14)...),
                o.a, spptr(state[1]), spptr(state[2]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]),
                dptr(sol), spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5]), dptr(alpha), dptr(out)))
    return out
end
# out12: the twelve of mu_error!; probe4: the four of amu_probe!, or nothing (LOQO); search: a FilterSearch on the same BarrierLayer, or nothing
function amu_update!(o::AdaptiveBarrierParameter, out12, probe4; force_fixed = false, search = nothing)
    check(ccall((:iem_amu_update, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cvoid}),
                o.a, dptr(out12), probe4 === nothing ? Ptr{Float64}(C_NULL) : dptr(probe4), force_fixed ? 1 : 0, search === nothing ? C_NULL : search.s))
end
# the one read-back (synchronises the stream once): (IemMuState, IemAmuState)
function amu_state(o::AdaptiveBarrierParameter)
    st = Ref(IemMuState(sizeof(IemMuState), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    own = Ref(IemAmuState(sizeof(IemAmuState), 0, 0, 0, (0.0, 0.0, 0.0, 0.0), 0, 0, 0, 0, 0, 0, 0))
    check(ccall((:iem_amu_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMuState}, Ptr{IemAmuState}), o.a, st, own))
    return st[], own[]
end
# the own block (16 words of 8 bytes) as a device address
function amu_device(o::AdaptiveBarrierParameter)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_amu_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), o.a, p))
    return p[]
end
# the affine-scaling calls of one iteration: the objects (bound to the parameter) are unbound around f and bound again — no launch either way
function amu_affine(f, o::AdaptiveBarrierParameter, objs...)
    foreach(x -> bind_mu!(x, nothing), objs)
    try
        return f()
    finally
        foreach(x -> bind_mu!(x, o.par), objs)
    end
end

# ---- the quality-function oracle (include/iem.h: iem_qf_*) ---------------------------------------------------------------------------
# Ipopt's mu_oracle = quality-function (2-norm squared, no centrality or balancing term) ON an AdaptiveBarrierParameter: a golden-section
# search over sigma whose state machine lives on the device.  Per iteration, in the place of amu_update!: mu_error!; amu_affine(...) do ...
# end around barrier_terms!(mu = 0) and barrier_terms!(mu = mu_ref), ONE two-column back-solve on the iteration's factors,
# barrier_step!(mu = 0, tau = 1) -> d0 and barrier_step!(mu = mu_ref, tau = 1) -> d1; qf_begin!; qf_section! (max_section_steps + 4
# qf_alpha! / qf_value! pairs, no decision in between); qf_update!(qf, out12; search); qf_state — the one read-back, three blocks.
# d0, d1 = (sol, ds, dzL, dzU, dvL, dvU).  Finalize (or let go of) the oracle before its AdaptiveBarrierParameter.  UNEXECUTED, like the rest.
struct IemQfOpts           # iem_qf_opts_t
    struct_size::UInt64
    mu_ref::Float64; sigma_min::Float64; sigma_max::Float64; section_sigma_tol::Float64
    max_section_steps::Int64      # 1..16
end
struct IemQfState          # iem_qf_state_t: words 0-26 of the object's own block
    struct_size::UInt64
    status::Int64; phase::Int64; steps::Int64; evaluations::Int64      # status: 0 idle, 1 section, 2 done, 3 unusable
    sigma_trial::Float64
    alpha_slots::NTuple{2, Float64}
    d2::Float64; p2::Float64; avg::Float64; lo::Float64; hi::Float64
    a::Float64; b::Float64; c::Float64; d::Float64; qc::Float64; qd::Float64
    sigma::Float64; q::Float64; q_first::Float64
    q_last::Float64; c2_last::Float64; nan_last::Float64; alpha_p_last::Float64; alpha_d_last::Float64
    sigma_first::Float64
end
mutable struct QualityFunction
    q::Ptr{Cvoid}
    amu::AdaptiveBarrierParameter      # borrowed: kept alive
    pairs::Int
end
function QualityFunction(o::AdaptiveBarrierParameter; mu_ref = 1.0, sigma_min = 1e-6, sigma_max = 0.0, section_sigma_tol = 1e-2, max_section_steps = 8)
    opts = Ref(IemQfOpts(sizeof(IemQfOpts), mu_ref, sigma_min, sigma_max, section_sigma_tol, max_section_steps))
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_qf_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemQfOpts}, Ptr{Ptr{Cvoid}}), o.a, opts, q))
    qf = QualityFunction(q[], o, max_section_steps + 4)
    finalizer(x -> (x.q == C_NULL || x.amu.a == C_NULL || ccall((:iem_qf_destroy, LIBIEM), Cint, (Ptr{Cvoid},), x.q); x.q = C_NULL), qf)
    return qf
end
# a new solve: the section idle (asynchronous); amu_reset! and mu_reset! are calls of their own
qf_reset!(o::QualityFunction) = check(ccall((:iem_qf_reset, LIBIEM), Cint, (Ptr{Cvoid},), o.q))
# r = sigma grad f + J'y, c = c(x), out12: the twelve of mu_error!
function qf_begin!(o::QualityFunction, state, r, c, out12)
    check(ccall((:iem_qf_begin, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 10)...),
                o.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]),
                dptr(r), spptr(c), dptr(out12)))
end
_qf_pair(state, d0, d1) = (spptr(state[1]), spptr(state[2]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]),
                           dptr(d0[1]), spptr(d0[2]), spptr(d0[3]), spptr(d0[4]), spptr(d0[5]), spptr(d0[6]),
                           dptr(d1[1]), spptr(d1[2]), spptr(d1[3]), spptr(d1[4]), spptr(d1[5]), spptr(d1[6]))
qf_alpha!(o::QualityFunction, state, d0, d1) =
    check(ccall((:iem_qf_alpha, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 18)...), o.q, _qf_pair(state, d0, d1)...))
qf_value!(o::QualityFunction, state, d0, d1) =
    check(ccall((:iem_qf_value, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 18)...), o.q, _qf_pair(state, d0, d1)...))
# every pair of a section: the pairs behind the one that finishes it do nothing on the device
function qf_section!(o::QualityFunction, state, d0, d1; pairs = o.pairs)
    for _ in 1:pairs
        qf_alpha!(o, state, d0, d1)
        qf_value!(o, state, d0, d1)
    end
end
# out12: the twelve of mu_error!; search: a FilterSearch on the same BarrierLayer, or nothing
function qf_update!(o::QualityFunction, out12; force_fixed = false, search = nothing)
    check(ccall((:iem_qf_update, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Cvoid}),
                o.q, dptr(out12), force_fixed ? 1 : 0, search === nothing ? C_NULL : search.s))
end
# the one read-back (synchronises the stream once): (IemMuState, IemAmuState, IemQfState)
function qf_state(o::QualityFunction)
    st = Ref(IemMuState(sizeof(IemMuState), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    mid = Ref(IemAmuState(sizeof(IemAmuState), 0, 0, 0, (0.0, 0.0, 0.0, 0.0), 0, 0, 0, 0, 0, 0, 0))
    own = Ref(IemQfState(sizeof(IemQfState), 0, 0, 0, 0, 0, (0.0, 0.0), ntuple(_ -> 0.0, 20)...))
    check(ccall((:iem_qf_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMuState}, Ptr{IemAmuState}, Ptr{IemQfState}), o.q, st, mid, own))
    return st[], mid[], own[]
end
# the own block (32 words of 8 bytes) as a device address
function qf_device(o::QualityFunction)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_qf_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), o.q, p))
    return p[]
end

# ---- Mehrotra's corrector (include/iem.h: iem_mpc_*) -----------------------------------------------------------------------------------
# The second-order term of the complementarity equations on the right-hand side, ON an AdaptiveBarrierParameter.  Per iteration, BEHIND
# amu_update! (or qf_update!), with the objects bound again: mpc_terms! (two columns: column 0 is barrier_terms!' rhs, column 1 carries
# mu − dgap_aff·dz_aff per bound); ONE two-column back-solve on the iteration's factors; barrier_step! on column 0; mpc_step! on column 1;
# amu_probe! on the corrected direction at alpha_c; mpc_select! — taken, the corrected direction is copied over the first-order one;
# mpc_state — the one read-back.  aff = (sol, ds, dzL, dzU, dvL, dvU) of the affine step.  Finalize (or let go of) the corrector before its
# AdaptiveBarrierParameter.  UNEXECUTED, like the rest.
struct IemMpcOpts          # iem_mpc_opts_t
    struct_size::UInt64
    red_fact::Float64
end
struct IemMpcState         # iem_mpc_state_t: words 0-6 of the object's own block
    struct_size::UInt64
    taken::Int64; n_taken::Int64; n_refused::Int64
    predicted::Float64; avg::Float64
    alpha_c::NTuple{2, Float64}
end
mutable struct MehrotraCorrector
    q::Ptr{Cvoid}
    amu::AdaptiveBarrierParameter      # borrowed: kept alive
end
function MehrotraCorrector(o::AdaptiveBarrierParameter; red_fact = 1.0)
    opts = Ref(IemMpcOpts(sizeof(IemMpcOpts), red_fact))
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_mpc_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMpcOpts}, Ptr{Ptr{Cvoid}}), o.a, opts, q))
    mpc = MehrotraCorrector(q[], o)
    finalizer(x -> (x.q == C_NULL || x.amu.a == C_NULL || ccall((:iem_mpc_destroy, LIBIEM), Cint, (Ptr{Cvoid},), x.q); x.q = C_NULL), mpc)
    return mpc
end
# a new solve: the block zero (asynchronous)
mpc_reset!(o::MehrotraCorrector) = check(ccall((:iem_mpc_reset, LIBIEM), Cint, (Ptr{Cvoid},), o.q))
# bound, mpc_terms! and mpc_step! read mu and tau from the parameter's block; nothing unbinds
bind_mu!(o::MehrotraCorrector, q) = check(ccall((:iem_mpc_bind_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), o.q, _mu_handle(q)))
_mpc_aff(aff) = (dptr(aff[1]), spptr(aff[2]), spptr(aff[3]), spptr(aff[4]), spptr(aff[5]), spptr(aff[6]))
# rhs2: 2·ld doubles on the device, column u at offset u·ld (ld >= nvar + ncon): the layout of solve_refined!
function mpc_terms!(o::MehrotraCorrector, state, r, c, aff, rhs2, ld; mu = 0.0)
    check(ccall((:iem_mpc_terms, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 15)..., Cdouble, Ptr{Float64}, Int64),
                o.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]),
                dptr(r), spptr(c), _mpc_aff(aff)..., mu, dptr(rhs2), ld))
    return rhs2
end
# sol_c: the corrected solution (column 1 of the solve); dirs_c = (ds, dzL, dzU, dvL, dvU) and alpha_c (two doubles) on the device
function mpc_step!(o::MehrotraCorrector, state, aff, sol_c, dirs_c, alpha_c; mu = 0.0, tau = 1.0)
    check(ccall((:iem_mpc_step, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 14)..., Cdouble, Cdouble, ntuple(_ -> Ptr{Float64}, 6)...),
                o.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]),
                _mpc_aff(aff)..., dptr(sol_c), mu, tau, spptr(dirs_c[1]), spptr(dirs_c[2]), spptr(dirs_c[3]), spptr(dirs_c[4]), spptr(dirs_c[5]), dptr(alpha_c)))
    return dirs_c, alpha_c
end
# probe4: the four of amu_probe! on the corrected direction; taken: (sol_c, dirs_c, alpha_c) over (sol, dirs, alpha)
function mpc_select!(o::MehrotraCorrector, probe4, alpha_c, sol_c, dirs_c, sol, dirs, alpha)
    check(ccall((:iem_mpc_select, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 15)...),
                o.q, dptr(probe4), dptr(alpha_c), dptr(sol_c), spptr(dirs_c[1]), spptr(dirs_c[2]), spptr(dirs_c[3]), spptr(dirs_c[4]), spptr(dirs_c[5]),
                dptr(sol), spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5]), dptr(alpha)))
end
# the one read-back (synchronises the stream once)
function mpc_state(o::MehrotraCorrector)
    own = Ref(IemMpcState(sizeof(IemMpcState), 0, 0, 0, 0.0, 0.0, (0.0, 0.0)))
    check(ccall((:iem_mpc_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemMpcState}), o.q, own))
    return own[]
end
# the own block (16 words of 8 bytes) as a device address
function mpc_device(o::MehrotraCorrector)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_mpc_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), o.q, p))
    return p[]
end

# ---- the starting point (include/iem.h: iem_init_*) -----------------------------------------------------------------------------------
# What stands in front of the first iteration, ON a BarrierLayer.  COLD, behind barrier_start!: init_ls_terms! (sigma = 1, dcon = 1 on
# inequality rows, the right-hand side of the least-squares multiplier estimate), assemble with a ZEROED Hessian value array, factor, one
# (refined) solve, init_ls_apply! (y += dy where max |y + dy| <= y_max, else y = 0 or y kept).  WARM, in the place of barrier_start!:
# init_warm! (the push of x and of the given s, the multipliers clamped, y clipped), the evaluation, mu_error!, init_mu! (mu0 from the
# average complementarity into the BarrierParameter's block).  init_state — the one read-back.  Finalize (or let go of) the starting
# point before its BarrierLayer.  UNEXECUTED, like the rest.
struct IemInitOpts         # iem_init_opts_t
    struct_size::UInt64
    y_max::Float64
    on_reject::Int64
    warm_push::Float64; warm_frac::Float64; warm_z_push::Float64; warm_z_max::Float64; warm_y_max::Float64
    mu_factor::Float64; mu_cap::Float64
end
struct IemInitState        # iem_init_state_t: words 0-5 of the object's own block
    struct_size::UInt64
    ynorm::Float64
    accepted::Int64; n_accepted::Int64; n_rejected::Int64
    mu0::Float64
    how::Int64             # 0 from the average, 1 fallback to mu_init, 2 clamped below, 3 clamped above
end
mutable struct StartingPoint
    q::Ptr{Cvoid}
    layer::BarrierLayer      # borrowed: kept alive
end
function StartingPoint(l::BarrierLayer; y_max = 1e3, on_reject = 0, warm_push = 1e-3, warm_frac = 1e-3, warm_z_push = 1e-3, warm_z_max = 1e6, warm_y_max = 1e6,
                       mu_factor = 1.0, mu_cap = 0.0)
    opts = Ref(IemInitOpts(sizeof(IemInitOpts), y_max, on_reject, warm_push, warm_frac, warm_z_push, warm_z_max, warm_y_max, mu_factor, mu_cap))
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_init_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemInitOpts}, Ptr{Ptr{Cvoid}}), l.b, opts, q))
    sp = StartingPoint(q[], l)
    finalizer(x -> (x.q == C_NULL || x.layer.b == C_NULL || ccall((:iem_init_destroy, LIBIEM), Cint, (Ptr{Cvoid},), x.q); x.q = C_NULL), sp)
    return sp
end
# a new solve: the block zero (asynchronous)
init_reset!(o::StartingPoint) = check(ccall((:iem_init_reset, LIBIEM), Cint, (Ptr{Cvoid},), o.q))
# state = (x, s, y, zL, zU, vL, vU); x and s are not read.  sigma (nvar), dcon (ncon), rhs (nvar + ncon) on the device
function init_ls_terms!(o::StartingPoint, state, r, sigma, dcon, rhs)
    check(ccall((:iem_init_ls_terms, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 9)...),
                o.q, spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(r), dptr(sigma), spptr(dcon), dptr(rhs)))
    return sigma, dcon, rhs
end
# sol = [w; dy] of the solve; y in place
function init_ls_apply!(o::StartingPoint, sol, y)
    check(ccall((:iem_init_ls_apply, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), o.q, dptr(sol), spptr(y)))
    return y
end
# the warm-start projection, in place
function init_warm!(o::StartingPoint, state)
    check(ccall((:iem_init_warm, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 7)...),
                o.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7])))
    return state
end
# out12: the twelve of mu_error! at the warm state; par: a BarrierParameter on the same BarrierLayer
init_mu!(o::StartingPoint, out12, par::BarrierParameter) = check(ccall((:iem_init_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}), o.q, dptr(out12), par.p))
# the one read-back (synchronises the stream once)
function init_state(o::StartingPoint)
    own = Ref(IemInitState(sizeof(IemInitState), 0.0, 0, 0, 0, 0.0, 0))
    check(ccall((:iem_init_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemInitState}), o.q, own))
    return own[]
end
# the own block (16 words of 8 bytes) as a device address
function init_device(o::StartingPoint)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_init_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), o.q, p))
    return p[]
end

# ---- the stopping test and the kept iterate (include/iem.h: iem_conv_*) ---------------------------------------------------------------
# What decides that a solve ends, ON a BarrierParameter (its tol, s_max, mu_floor and block).  Per iteration: mu_error!, conv_check!
# (status, keep), conv_keep! (copies iff the check asked for it), mu_update!, conv_state — the one read-back; behind barrier_step!
# conv_step! (the tiny step).  A status other than 0 is latched until conv_reset!; conv_restore! hands the kept point back.  Finalize (or
# let go of) the object before its BarrierParameter.  UNEXECUTED, like the rest.
struct IemConvOpts         # iem_conv_opts_t
    struct_size::UInt64
    dual_inf_tol::Float64; constr_viol_tol::Float64; compl_inf_tol::Float64
    acceptable_tol::Float64
    acceptable_iter::Int64
    acceptable_dual_inf_tol::Float64; acceptable_constr_viol_tol::Float64; acceptable_compl_inf_tol::Float64; acceptable_obj_change_tol::Float64
    max_iter::Int64
    diverging_iterates_tol::Float64
    tiny_step_tol::Float64; tiny_step_y_tol::Float64
end
struct IemConvState        # iem_conv_state_t: words 0-18 of the object's own block
    struct_size::UInt64
    status::Int64          # 0 iterating, 1 converged, 2 acceptable, 3 maxiter, 4 diverging, 5 invalid, 6 tiny step
    checks::Int64; acceptable_count::Int64; keep::Int64; kept::Int64; kept_at::Int64
    flags::Int64           # bit 0 acceptable now, bit 1 this step tiny, bit 2 tiny with mu above its floor
    tiny_count::Int64
    e0::Float64; dual_inf::Float64; constr_viol::Float64; compl_inf::Float64; f::Float64; f_prev::Float64; xmax::Float64
    kept_e0::Float64; kept_f::Float64; rel::Float64; dymax::Float64
end
mutable struct ConvergenceCheck
    q::Ptr{Cvoid}
    par::BarrierParameter      # borrowed: kept alive
end
function ConvergenceCheck(par::BarrierParameter; dual_inf_tol = 1.0, constr_viol_tol = 1e-4, compl_inf_tol = 1e-4, acceptable_tol = 1e-6, acceptable_iter = 15,
                          acceptable_dual_inf_tol = 1e10, acceptable_constr_viol_tol = 1e-2, acceptable_compl_inf_tol = 1e-2, acceptable_obj_change_tol = 1e20,
                          max_iter = 3000, diverging_iterates_tol = 1e20, tiny_step_tol = 10.0 * eps(Float64), tiny_step_y_tol = 1e-2)
    opts = Ref(IemConvOpts(sizeof(IemConvOpts), dual_inf_tol, constr_viol_tol, compl_inf_tol, acceptable_tol, acceptable_iter, acceptable_dual_inf_tol,
                           acceptable_constr_viol_tol, acceptable_compl_inf_tol, acceptable_obj_change_tol, max_iter, diverging_iterates_tol, tiny_step_tol, tiny_step_y_tol))
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_conv_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemConvOpts}, Ptr{Ptr{Cvoid}}), par.p, opts, q))
    cc = ConvergenceCheck(q[], par)
    finalizer(x -> (x.q == C_NULL || x.par.p == C_NULL || ccall((:iem_conv_destroy, LIBIEM), Cint, (Ptr{Cvoid},), x.q); x.q = C_NULL), cc)
    return cc
end
# a new solve: the block zero, the kept buffers keep their bytes (asynchronous)
conv_reset!(o::ConvergenceCheck) = check(ccall((:iem_conv_reset, LIBIEM), Cint, (Ptr{Cvoid},), o.q))
# out12: the twelve of mu_error!; f: the objective, one double on the device; x: the variables
conv_check!(o::ConvergenceCheck, out12, f, x) = check(ccall((:iem_conv_check, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), o.q, dptr(out12), dptr(f), spptr(x)))
# state = (x, s, y, zL, zU, vL, vU): copied into the object's buffers iff the last conv_check! asked for it
function conv_keep!(o::ConvergenceCheck, state)
    check(ccall((:iem_conv_keep, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 7)...),
                o.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7])))
end
# the kept point into state, in place, iff one is held: only the entries conv_keep! reads are written
function conv_restore!(o::ConvergenceCheck, state)
    check(ccall((:iem_conv_restore, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 7)...),
                o.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7])))
    return state
end
# behind the solve of the direction: sol = [dx; dy], ds the slack direction of barrier_step!
conv_step!(o::ConvergenceCheck, x, s, sol, ds) = check(ccall((:iem_conv_step, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 4)...), o.q, spptr(x), spptr(s), dptr(sol), spptr(ds)))
# the kept point (x, s, y, zL, zU, vL, vU) as device addresses into the object's own buffers
function conv_kept(o::ConvergenceCheck)
    p = ntuple(_ -> Ref{Ptr{Float64}}(C_NULL), 7)
    check(ccall((:iem_conv_kept, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Ptr{Float64}}, 7)...), o.q, p...))
    return map(r -> r[], p)
end
# the one read-back (synchronises the stream once)
function conv_state(o::ConvergenceCheck)
    own = Ref(IemConvState(sizeof(IemConvState), 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    check(ccall((:iem_conv_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemConvState}), o.q, own))
    return own[]
end
# the own block (24 words of 8 bytes) as a device address
function conv_device(o::ConvergenceCheck)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_conv_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), o.q, p))
    return p[]
end

# ---- the feasibility restoration phase (include/iem.h: iem_resto_*) ------------------------------------------------------------------
# Step A-9 of Waechter and Biegler 2006 beside the FilterSearch of the ORIGINAL problem: resto_enter! when its search ended FAILED, then
# per iteration eval_residual (obj_weight 0), resto_error!, jac_hess_coord (0), resto_terms!, assemble / factor / solve_refined!,
# resto_step!, resto_merit!(0), resto_begin!, K x (resto_trial!, cons, resto_merit!(1), search_accept! on resto.inner),
# resto_update!, obj, cons, barrier_merit!, resto_check!; resto_leave! once resto_state says RETURN.  zeta = sqrt(mu).  UNEXECUTED, like the rest.
struct IemRestoOpts        # iem_resto_opts_t
    struct_size::UInt64
    rho::Float64; kappa_resto::Float64; bound_mult_reset_threshold::Float64
end
struct IemRestoState       # iem_resto_state_t: words 0-3 of the object's block
    struct_size::UInt64
    state::Int64      # 0 none, 1 active, 2 return
    theta_start::Float64; theta::Float64; phi::Float64
end
mutable struct Restoration
    q::Ptr{Cvoid}
    search::FilterSearch      # the ORIGINAL problem's, borrowed: kept alive
    inner::Ptr{Cvoid}         # the restoration problem's own search: owned by the object
end
function Restoration(f::FilterSearch; rho = 1000.0, kappa_resto = 0.9, bound_mult_reset_threshold = 1000.0)
    opts = Ref(IemRestoOpts(sizeof(IemRestoOpts), rho, kappa_resto, bound_mult_reset_threshold))
    q, inner = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_resto_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemRestoOpts}, Ptr{Ptr{Cvoid}}), f.s, opts, q))
    check(ccall((:iem_resto_search, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), q[], inner))
    r = Restoration(q[], f, inner[])
    finalizer(c -> (c.q == C_NULL || ccall((:iem_resto_destroy, LIBIEM), Cint, (Ptr{Cvoid},), c.q); c.q = C_NULL), r)
    return r
end
# mu: max(mu, max |inf|) — out[3] of barrier_error!
resto_enter!(r::Restoration, state, cons, mu) =
    check(ccall((:iem_resto_enter, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble), r.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), spptr(cons), mu))
function resto_terms!(r::Restoration, state, res, cons, mu, zeta, sigma, dcon, rhs)
    check(ccall((:iem_resto_terms, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                r.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), spptr(res), spptr(cons), mu, zeta, spptr(sigma), spptr(dcon), dptr(rhs)))
    return sigma, dcon, rhs
end
function resto_step!(r::Restoration, state, sol, mu, tau, zeta, dirs, alpha)
    check(ccall((:iem_resto_step, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                r.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(sol), mu, tau, zeta, spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5]), dptr(alpha)))
    return dirs, alpha
end
# which = 0: at the state with (p, n); 1: at the trial point with (pt, nt).  out: three doubles
function resto_merit!(r::Restoration, which, x, s, cons, zeta, out)
    check(ccall((:iem_resto_merit, LIBIEM), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}), r.q, which, spptr(x), spptr(s), spptr(cons), zeta, dptr(out)))
    return out
end
resto_begin!(r::Restoration, state, sol, ds, merit0, alpha, mu, zeta) =
    check(ccall((:iem_resto_begin, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                r.q, spptr(state[1]), spptr(state[2]), dptr(sol), spptr(ds), dptr(merit0), dptr(alpha), mu, zeta))
function resto_trial!(r::Restoration, state, sol, ds, xt, st)
    check(ccall((:iem_resto_trial, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                r.q, spptr(state[1]), spptr(state[2]), dptr(sol), spptr(ds), spptr(xt), spptr(st)))
    return xt, st
end
# the restoration's acceptance test: iem_search_accept on the inner search, with merit = the three of resto_merit!(1)
resto_accept!(r::Restoration, merit, mu, alpha) =
    check(ccall((:iem_search_accept, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}), r.inner, dptr(merit), dptr(merit) + 8, mu, 1.0, dptr(alpha)))
resto_reset!(r::Restoration) = check(ccall((:iem_search_reset, LIBIEM), Cint, (Ptr{Cvoid},), r.inner))
function resto_update!(r::Restoration, state, sol, dirs, alpha, mu; kappa_sigma = 1e10)
    check(ccall((:iem_resto_update, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                r.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), dptr(sol), spptr(dirs[1]), spptr(dirs[2]), spptr(dirs[3]), spptr(dirs[4]), spptr(dirs[5]), dptr(alpha), mu, kappa_sigma))
    return state
end
# res may be nothing (out[1] is NaN then); out: eight doubles in the layout of barrier_error!
function resto_error!(r::Restoration, state, res, cons, mu, zeta, out)
    check(ccall((:iem_resto_error, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}),
                r.q, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), spptr(res), spptr(cons), mu, zeta, dptr(out)))
    return out
end
# f: one double on the device, merit: the two of barrier_merit! at the new iterate, mu: the ORIGINAL problem's
resto_check!(r::Restoration, f, merit, mu) = check(ccall((:iem_resto_check, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble), r.q, dptr(f), dptr(merit), mu))
resto_leave!(r::Restoration, state) =
    check(ccall((:iem_resto_leave, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), r.q, spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7])))
# the one read-back (synchronises the stream)
function resto_state(r::Restoration)
    st = Ref(IemRestoState(sizeof(IemRestoState), 0, 0, 0, 0))
    check(ccall((:iem_resto_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemRestoState}), r.q, st))
    return st[]
end
# (p, n, zp, zn, block) as device addresses; the object's vectors are one allocation in the order of include/iem.h
function resto_device(r::Restoration)
    p = [Ref{Ptr{Float64}}(C_NULL) for _ in 1:4]
    blk = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_resto_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}), r.q, p[1], p[2], p[3], p[4], blk))
    return p[1][], p[2][], p[3][], p[4][], blk[]
end

# ---- the restoration phase's barrier parameter (include/iem.h: iem_rmu_*, iem_resto_bind_mu) -----------------------------------------
# The restoration problem's own mu ON a Restoration: rmu_enter! in front of resto_enter! (mu_R = max(mu, max |inf|) on the device), per
# iteration rmu_error! (32 words: resto_error! at mu = 0, the products' extremes, six candidates) and rmu_update! (the monotone rule,
# STATIONARY, the inner filter emptied iff mu moved), rmu_trigger! behind every accept (Ipopt's alpha_min), rmu_state — the one
# read-back.  bind_mu!(r, rp) makes every resto_*! call read mu, tau and zeta from the restoration block (their scalar arguments are
# then ignored); rmu_bind_inner! binds the inner search to the same block.  Finalize (or let go of) the object before its Restoration.
# UNEXECUTED, like the rest.
struct IemRmuOpts          # iem_rmu_opts_t
    struct_size::UInt64
    kappa_eps::Float64; kappa_mu::Float64; tau_min::Float64; tol::Float64; mu_floor::Float64; s_max::Float64; gamma_alpha::Float64
end
struct IemRmuState         # iem_rmu_state_t: the own block, the restoration block, the block of the Restoration
    struct_size::UInt64
    status::Int64          # 0 iterating, 1 stationary, 2 unusable
    flags::Int64           # bit 0 mu changed in the last update, bit 1 its ladder was truncated
    decreases_last::Int64; decreases::Int64
    e0::Float64; e_mu::Float64; mu_enter::Float64; inf_enter::Float64; alpha_min::Float64
    triggers_orig::Int64; triggers_inner::Int64
    mu::Float64; tau::Float64; zeta::Float64; mu_e0::Float64; mu_e_mu::Float64; mu_e_d::Float64; mu_e_p::Float64; mu_e_c0::Float64
    mu_status::Int64; mu_flags::Int64; mu_decreases::Int64; mu_updates::Int64
    resto_state::Int64     # 0 none, 1 active, 2 return
    theta_start::Float64; theta::Float64; phi::Float64
end
const RMU_K = 6            # IEM_RMU_K: the candidates of one update
mutable struct RestorationParameter
    rp::Ptr{Cvoid}
    resto::Restoration                       # borrowed: kept alive
    orig::Union{Nothing, BarrierParameter}   # the ORIGINAL problem's parameter, borrowed: kept alive
    inner_mu::Ptr{Cvoid}                     # the restoration block's iem_mu object: owned by the object
end
function RestorationParameter(r::Restoration, orig::Union{Nothing, BarrierParameter} = nothing; kappa_eps = 10.0, kappa_mu = 0.2, tau_min = 0.99, tol = 1e-8,
                              mu_floor = 1e-11, s_max = 100.0, gamma_alpha = 0.05)
    opts = Ref(IemRmuOpts(sizeof(IemRmuOpts), kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max, gamma_alpha))
    rp, par = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:iem_rmu_create, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{IemRmuOpts}, Ptr{Ptr{Cvoid}}), r.q, orig === nothing ? C_NULL : orig.p, opts, rp))
    check(ccall((:iem_rmu_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), rp[], par))
    o = RestorationParameter(rp[], r, orig, par[])
    finalizer(x -> (x.rp == C_NULL || x.resto.q == C_NULL || ccall((:iem_rmu_destroy, LIBIEM), Cint, (Ptr{Cvoid},), x.rp); x.rp = C_NULL), o)
    return o
end
# err: the eight of barrier_error! (or the first eight of mu_error!) at this point; mu is ignored where an original parameter was given
rmu_enter!(o::RestorationParameter, err, mu = 0.0) = check(ccall((:iem_rmu_enter, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cdouble), o.rp, dptr(err), mu))
# out: 32 doubles; res is required
function rmu_error!(o::RestorationParameter, state, res, cons, out)
    check(ccall((:iem_rmu_error, LIBIEM), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 10)...),
                o.rp, spptr(state[1]), spptr(state[2]), spptr(state[3]), spptr(state[4]), spptr(state[5]), spptr(state[6]), spptr(state[7]), spptr(res), spptr(cons), dptr(out)))
    return out
end
rmu_update!(o::RestorationParameter, out32) = check(ccall((:iem_rmu_update, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Float64}), o.rp, dptr(out32)))
# which = 0: the original search of the Restoration, 1: its inner search; alpha: that search's step lengths
rmu_trigger!(o::RestorationParameter, which, alpha) = check(ccall((:iem_rmu_trigger, LIBIEM), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), o.rp, which, dptr(alpha)))
# the one read-back (one copy, synchronises the stream once)
function rmu_state(o::RestorationParameter)
    st = Ref(IemRmuState(sizeof(IemRmuState), 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0))
    check(ccall((:iem_rmu_state, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{IemRmuState}), o.rp, st))
    return st[]
end
# the own block (16 words of 8 bytes) as a device address
function rmu_device(o::RestorationParameter)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:iem_rmu_device, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), o.rp, p))
    return p[]
end
# bind (or, with nothing, unbind) the Restoration: the first bind of a handle loads a code object, so bind outside a capture
bind_mu!(r::Restoration, o::Union{Nothing, RestorationParameter}) =
    check(ccall((:iem_resto_bind_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), r.q, o === nothing ? C_NULL : o.rp))
# ... and its inner search, to the restoration block (unbind = false) or to nothing
rmu_bind_inner!(o::RestorationParameter; unbind = false) =
    check(ccall((:iem_search_bind_mu, LIBIEM), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), o.resto.inner, unbind ? C_NULL : o.inner_mu))

# ---- blob writer ----------------------------------------------------------------------------
# Serialises a host ExaCore into the wire format of include/iem_blob.h.  [EXT]: the field and
# type names of ExaModels' internal structs (Objective/Constraint linked lists, SIMDFunction,
# Node1/Node2/Var/ParameterNode, the data-source leaf types) are matched by NAME through
# `nameof(typeof(·))`, so that a rename between ExaModels versions (ParSource/ParIndexed in
# 0.9-0.10, DataSource/DataIndexed in 0.11) needs a one-line change in the sets below.
#
# Node mapping (ExaModels graph types → opcodes of iem_blob.h):
#   Var{I}            → IEM_OP_VAR  + affine index expression over Int item fields
#   ParameterNode{I}  → IEM_OP_PAR  + affine index expression
#   data-indexed leaf → IEM_OP_DATA on a Float64 item column
#   Real              → IEM_OP_CONST
#   Node1{F}          → unary opcode of F;  Node2{F} → binary opcode of F
# Items (`itr`, any iterable of NamedTuples / tuples / scalars) become explicit columns; a column
# that is an arithmetic progression is written as an AFFINE field (no payload), anything else as
# a GATHER field.  Templates whose first Int column is the progression b+1, b+2, … are placed on
# fusion grid 1 with origin b (a scheduling hint only: results never depend on it).

const _SRC_NAMES = (:ParSource, :DataSource)
const _IDX_NAMES = (:ParIndexed, :DataIndexed)
const _BINOP = Dict{Any,Int}(+ => 10, - => 11, * => 12, / => 13, ^ => 14)
const _UNOP = Dict{Any,Int}(
    - => 20, + => 21, inv => 22, sqrt => 23, cbrt => 24, abs => 25, abs2 => 26, exp => 27, exp2 => 28,
    log => 29, log2 => 30, log10 => 31, log1p => 32, sin => 33, cos => 34, tan => 35, asin => 36,
    acos => 37, csc => 38, sec => 39, cot => 40, atan => 41, acot => 42, sind => 43, cosd => 44,
    tand => 45, cscd => 46, secd => 47, cotd => 48, atand => 49, acotd => 50, sinh => 51, cosh => 52,
    tanh => 53, csch => 54, sech => 55, coth => 56, atanh => 57, acoth => 58)

_tname(e) = nameof(typeof(e))
_fn_of(e) = typeof(e).parameters[1].instance            # Node1{F,…} / Node2{F,…}: F = typeof(f)
_w(x::Integer) = reinterpret(UInt64, Int64(x))
_w(x::AbstractFloat) = reinterpret(UInt64, Float64(x))

# key of a data leaf: the chain of getindex/getproperty selectors from the source, e.g. (:t,) or (2, 1)
function _leaf_key(e)
    _tname(e) in _SRC_NAMES && return ()
    _tname(e) in _IDX_NAMES || error("to_blob: not a data leaf: $(typeof(e))")
    return (_leaf_key(getfield(e, :inner))..., typeof(e).parameters[2])
end
_select(item, key::Tuple) = isempty(key) ? item : _select(_pick(item, key[1]), Base.tail(key))
_pick(item, k::Symbol) = getproperty(item, k)
_pick(item, k) = getindex(item, k)

mutable struct _Arrays
    recs::Vector{NTuple{5,Any}}        # (kind, n, payload | nothing, a, b)
    seen::Dict{Any,Int}
end
function _add_array!(A::_Arrays, v::AbstractVector)
    v = v isa AbstractVector{<:Integer} ? collect(Int64, v) : collect(Float64, v)
    if eltype(v) == Float64 && !isempty(v) && all(==(v[1]), v) && !isnan(v[1])
        key = (:fill, length(v), v[1])
        return get!(A.seen, key) do
            push!(A.recs, (2, length(v), nothing, _w(v[1]), UInt64(0))); length(A.recs) - 1
        end
    end
    key = (eltype(v), hash(v), length(v))
    return get!(A.seen, key) do
        push!(A.recs, (eltype(v) == Float64 ? 0 : 1, length(v), v, UInt64(0), UInt64(0))); length(A.recs) - 1
    end
end

mutable struct _Tpl
    items::Vector{Any}
    A::_Arrays
    icol::Dict{Any,Int}; fcol::Dict{Any,Int}
    ifields::Vector{Vector{UInt64}}; ffields::Vector{Vector{UInt64}}
    idx::Vector{Vector{UInt64}}
    nodes::Vector{NTuple{4,UInt64}}
    first_ap::Union{Nothing,Int64}      # base of the first unit-step Int column (fusion hint)
end

function _column_field(T::_Tpl, col::Vector, asint::Bool)
    n = length(col)
    if asint
        c = collect(Int64, col)
        step = n > 1 ? c[2] - c[1] : 0
        if all(k -> c[k] == c[1] + step * (k - 1), 1:n)
            step == 1 && T.first_ap === nothing && (T.first_ap = c[1] - 1)
            return UInt64[_w(0), _w(c[1]), _w(step), _w(0), _w(0), _w(-1)]         # AFFINE
        end
        return UInt64[_w(1), _w(0), _w(1), _w(0), _w(0), _w(_add_array!(T.A, c))]    # GATHER, k-th entry
    end
    return UInt64[_w(1), _w(0), _w(1), _w(0), _w(0), _w(_add_array!(T.A, collect(Float64, col)))]
end
function _ifield!(T::_Tpl, key)
    get!(T.icol, key) do
        push!(T.ifields, _column_field(T, [_select(it, key) for it in T.items], true)); length(T.ifields) - 1
    end
end
function _ffield!(T::_Tpl, key)
    get!(T.fcol, key) do
        push!(T.ffields, _column_field(T, [_select(it, key) for it in T.items], false)); length(T.ffields) - 1
    end
end

# affine index algebra: value = c0 + Σ coef·field
function _affine(T::_Tpl, e)
    e isa Integer && return (Int64(e), Dict{Int,Int64}())
    n = _tname(e)
    (n in _IDX_NAMES || n in _SRC_NAMES) && return (Int64(0), Dict(_ifield!(T, _leaf_key(e)) => Int64(1)))
    if n == :Node2
        f = _fn_of(e); a = getfield(e, :inner1); b = getfield(e, :inner2)
        if f === (+) || f === (-)
            (ca, ta), (cb, tb) = _affine(T, a), _affine(T, b); s = f === (+) ? 1 : -1
            for (k, v) in tb; ta[k] = get(ta, k, 0) + s * v; end
            return (ca + s * cb, ta)
        elseif f === (*) && (a isa Integer || b isa Integer)
            k, (c, t) = a isa Integer ? (a, _affine(T, b)) : (b, _affine(T, a))
            return (k * c, Dict(i => k * v for (i, v) in t))
        end
    elseif n == :Node1 && _fn_of(e) === (-)
        c, t = _affine(T, getfield(e, :inner)); return (-c, Dict(i => -v for (i, v) in t))
    end
    error("to_blob: index expression is not affine in the item fields: $(typeof(e))")
end
function _idx!(T::_Tpl, e)
    c0, terms = _affine(T, e)
    filter!(p -> p.second != 0, terms)
    length(terms) <= 3 || error("to_blob: more than IEM_MAX_IDX_TERMS item fields in one index")
    w = UInt64[_w(c0), _w(length(terms))]
    for (fid, coef) in sort!(collect(terms)); push!(w, _w(fid), _w(coef)); end
    append!(w, fill(UInt64(0), 2 * (3 - length(terms))))
    push!(T.idx, w); return length(T.idx) - 1
end

_node!(T, op, a = 0, b = 0, imm = 0.0) = (push!(T.nodes, (_w(op), _w(a), _w(b), _w(Float64(imm)))); length(T.nodes) - 1)
function _walk!(T::_Tpl, e)
    e isa Real && return _node!(T, 0, 0, 0, e)
    n = _tname(e)
    n == :Null && return _node!(T, 0, 0, 0, something(getfield(e, :value), 0.0))
    n == :Var && return _node!(T, 3, _idx!(T, getfield(e, :i)))
    n == :ParameterNode && return _node!(T, 2, _idx!(T, getfield(e, :i)))
    (n in _IDX_NAMES || n in _SRC_NAMES) && return _node!(T, 1, _ffield!(T, _leaf_key(e)))
    if n == :Node1
        a = _walk!(T, getfield(e, :inner))
        return _node!(T, get(() -> error("to_blob: unary operator $(_fn_of(e)) has no opcode"), _UNOP, _fn_of(e)), a)
    elseif n == :Node2
        a = _walk!(T, getfield(e, :inner1)); b = _walk!(T, getfield(e, :inner2))
        return _node!(T, get(() -> error("to_blob: binary operator $(_fn_of(e)) has no opcode"), _BINOP, _fn_of(e)), a, b)
    end
    error("to_blob: unsupported expression node $(typeof(e))")
end

# linked list (newest first, `.inner` = previous) → call order
function _chain(head)
    out = Any[]
    while hasfield(typeof(head), :f) && hasfield(typeof(head), :itr)
        pushfirst!(out, head); head = getfield(head, :inner)
    end
    return out
end

# `slabs`  (optional, needed by iem_create_sharded): one `(offset0, dims, groups)` per `add_var` slab in
#          creation order — what `data.infvar_mappings` / `finvar_mappings` hold (`Variable.offset/.size`,
#          src/infiniteopt_backend.jl:476-479) plus the parameter-group index of each axis (0 = none);
# `template_groups` (optional): the parameter-group index of each template's (1-D) iterator in
#          add_obj/add_con call order, 0 = none — becomes the grid hint the window cut keys on.
# UNEXECUTED like the rest of this file.  Product iterators (pandemic's t x xi) reach the library as
# flat lists and are recovered as lattices without group ids: sharding them needs the Python producer.
function to_blob(core; slabs = nothing, template_groups = nothing)::Vector{UInt8}
    A = _Arrays(NTuple{5,Any}[], Dict{Any,Int}())
    core_ids = [_add_array!(A, Array(core.x0)), _add_array!(A, Array(core.lvar)),
                _add_array!(A, Array(core.uvar)), _add_array!(A, Array(core.θ))]
    lcon, ucon = Array(core.lcon), Array(core.ucon)
    objs, cons = _chain(core.obj), _chain(core.con)
    # add_obj/add_con CALL order decides the Hessian block offsets: merge the two lists by o2
    order = Tuple{Int,Any}[]
    i = j = 1
    while i <= length(objs) || j <= length(cons)
        takeobj = j > length(cons) || (i <= length(objs) && objs[i].f.o2 <= cons[j].f.o2)
        takeobj ? (push!(order, (0, objs[i])); i += 1) : (push!(order, (1, cons[j])); j += 1)
    end
    tpls = Vector{Vector{UInt64}}()
    for (kind, t) in order
        items = collect(Any, t.itr)
        T = _Tpl(items, A, Dict{Any,Int}(), Dict{Any,Int}(), [], [], [], NTuple{4,UInt64}[], nothing)
        root = _walk!(T, t.f.f)
        n = length(items)
        gid, origin = T.first_ap === nothing ? (n == 1 ? (0, 0) : (-1, 0)) : (4096 + 1, T.first_ap)
        if template_groups !== nothing && T.first_ap !== nothing && template_groups[length(tpls) + 1] > 0
            gid = template_groups[length(tpls) + 1] + 1          # one digit, base 4096: (group + 1)
        end
        w = UInt64[_w(kind), _w(n), _w(1), _w(n), _w(1), _w(1), _w(gid), _w(origin), _w(0), _w(0),
                   _w(length(T.ifields)), _w(length(T.ffields)), _w(length(T.idx)), _w(length(T.nodes)), _w(root)]
        if kind == 1
            rows = (t.f.o0 + 1):(t.f.o0 + n)
            append!(w, [_w(1), _w(0), _w(_add_array!(A, lcon[rows])), _w(1), _w(0), _w(_add_array!(A, ucon[rows]))])
        else
            append!(w, [_w(0), _w(0.0), _w(-1), _w(0), _w(0.0), _w(-1)])
        end
        foreach(f -> append!(w, f), T.ifields); foreach(f -> append!(w, f), T.ffields)
        foreach(x -> append!(w, x), T.idx)
        for nd in T.nodes; append!(w, nd); end
        push!(tpls, w)
    end
    narr, ntpl = length(A.recs), length(tpls)
    pos = 14 + 6 * narr + ntpl
    tpl_off = Int[]; for w in tpls; push!(tpl_off, pos); pos += length(w); end
    slab_words = UInt64[]
    if slabs !== nothing                                       # include/iem_blob.h: n, then n x {off, nd, dims[3], group[3]}
        push!(slab_words, _w(length(slabs)))
        for (off, dims, groups) in slabs
            nd = length(dims)
            append!(slab_words, _w.([off, nd, dims..., ones(Int, 3 - nd)..., groups..., zeros(Int, 3 - nd)...]))
        end
    end
    slab_off = isempty(slab_words) ? 0 : pos
    pos += length(slab_words)
    arr_off = Int[]; for r in A.recs; push!(arr_off, r[3] === nothing ? 0 : pos); r[3] === nothing || (pos += r[2]); end
    head = UInt64[_w(0x31424f4c424d4549), _w(1), _w(core.nvar), _w(core.npar), _w(core.ncon), _w(ntpl), _w(narr),
                  _w(core.minimize ? 1 : 0), _w(pos), _w(slab_off), _w.(core_ids)...]
    for (r, off) in zip(A.recs, arr_off); append!(head, [_w(r[1]), _w(r[2]), _w(off), r[4], r[5], _w(0)]); end
    append!(head, _w.(tpl_off)); foreach(w -> append!(head, w), tpls)
    append!(head, slab_words)
    for r in A.recs
        r[3] === nothing || append!(head, reinterpret(UInt64, r[3]))
    end
    @assert length(head) == pos
    return collect(reinterpret(UInt8, head))
end

end # module
