// The expression-defined "function" state: parser, postfix program and interpreter.
//
// Reference: source/{euler,shallow_water,scalar_conservation}/initial_state_function.h evaluate one
// dealii::FunctionParser (muparser) per primitive component at (x, t). Neither library is used here: this is an own
// recursive-descent parser for the subset of that grammar tabulated in include/ryujin_hip.h ("The function state"),
// compiled once into a flat postfix program of fixed-size instructions that ONE interpreter body, expr_evaluate(),
// runs on the host (ryujin_hip_expression_evaluate, tests/cpp/expression_cases.cc) and on the device
// (initial_states_device.hpp). The flux of the scalar conservation equation (FluxLibrary "function", one string in the
// variable u with a component per direction) is its second consumer: flux_compile() and flux_evaluate_points() at the
// end of this file, the kernels in scalar_conservation_device.hpp. The equation of state "function" of EulerAEOS
// (EquationOfStateLibrary, four strings in rho and e, or rho and p) is the third: eos_compile() and
// eos_evaluate_points() behind the flux, the kernels in kernels_euler_aeos.hpp and kernels_initial_values.hpp.
// Host standard library only -- no HIP, no context. Under hipcc RYUJIN_EXPR_HD makes the
// interpreter a host and device function; the parser is host code.
//
// The interpreter keeps the top of the operand stack in a register and everything below it behind a `Stack`
// (load(slot) / store(slot, value)): an array on the host, a [slot][lane] column of LDS on the device, where a
// run-time-indexed private array would live in scratch memory. The program is the same for every lane, so on the
// device every branch of the interpreter is wave-uniform. `pow_fn` is std::pow on the host and the library's dev_pow
// on the device; everything else is the same source line on both sides. + - * /, sqrt, comparisons, selection,
// rounding and the power rewrite (^ with the literal exponent 2, 3, 4) are exactly rounded or exact, so they give the
// same bits on both sides in a build with -ffp-contract=off.
#ifndef RYUJIN_HIP_EXPRESSION_HPP
#define RYUJIN_HIP_EXPRESSION_HPP

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>

#ifndef RYUJIN_EXPR_MAX_INSTRUCTIONS /* ryujin_hip.h, repeated so that this header stands alone */
#define RYUJIN_EXPR_MAX_INSTRUCTIONS 256
#endif
#ifndef RYUJIN_EXPR_MAX_STACK
#define RYUJIN_EXPR_MAX_STACK 16
#endif

#if defined(__HIPCC__)
#define RYUJIN_EXPR_HD __host__ __device__ __forceinline__
#else
#define RYUJIN_EXPR_HD inline
#endif

namespace ryujin_hip
{
  /* RYUJIN_OK, RYUJIN_ERR_ARG, RYUJIN_ERR_UNSUPPORTED of ryujin_hip.h */
  constexpr int kExprOk = 0, kExprErrArg = -2, kExprErrUnsupported = -5;

  constexpr int kExprMaxNesting = 64; /* parentheses and function calls inside one another (host recursion) */

  enum ExprOp : int {
    kExConst = 0, /* push value */
    kExVar,       /* push variable `slot`: 0 x, 1 y, 2 z, 3 t (the flux: 0 u) */
    /* two operands */
    kExAdd, kExSub, kExMul, kExDiv,
    kExPow,                                   /* a ^ b and pow(a, b) through pow_fn */
    kExLt, kExGt, kExLe, kExGe, kExEq, kExNe, /* 1.0 or 0.0 */
    kExAnd, kExOr,                            /* && ||: operands tested != 0 */
    kExAndRounded, kExOrRounded,              /* & |: operands rounded to the nearest integer first */
    kExMin, kExMax,
    /* three operands, all evaluated, then selected */
    kExSelect,        /* c ? a : b: c tested != 0 */
    kExSelectRounded, /* if(c, a, b): c rounded first */
    /* one operand */
    kExNeg,
    kExPow2, kExPow3, kExPow4, /* ^ with the literal exponent 2, 3, 4: a*a, a*a*a, a*a*a*a, left to right */
    kExSin, kExCos, kExTan, kExAsin, kExAcos, kExAtan, kExSinh, kExCosh, kExTanh, kExAsinh, kExAcosh, kExAtanh,
    kExExp, kExLog, kExLog2, kExLog10, kExSqrt, kExAbs, kExSign, kExRint, kExFloor, kExCeil, kExInt,
    kExCot, kExCsc, kExSec, kExErf, kExErfc,
    /* never emitted by the parser: ends one program of several run back to back (the components of a state):
     * the value goes to slot RYUJIN_EXPR_MAX_STACK + `slot` of the stack, which then has that many more slots */
    kExResult
  };

  struct ExprInstruction {
    int op;
    int slot;     /* kExVar */
    double value; /* kExConst */
  };

  struct ExprProgram {
    int n = 0;     /* instructions */
    int depth = 0; /* the largest number of operands alive at once, <= RYUJIN_EXPR_MAX_STACK */
    ExprInstruction code[RYUJIN_EXPR_MAX_INSTRUCTIONS];
  };

  /* nearest integer, halves away from zero (the rounding deal.II puts in front of if, |, & and int) */
  RYUJIN_EXPR_HD double expr_round(const double v)
  {
    return ::trunc(v + (v >= 0. ? 0.5 : -0.5));
  }

  /* The value of the program at (x, y, z, t). `stack` holds the operands below the top one: slots 0 .. depth - 1. */
  template <typename Stack, typename Pow>
  RYUJIN_EXPR_HD double expr_evaluate(const ExprInstruction *code, const int n, const double x, const double y,
                                      const double z, const double t, Stack &stack, Pow pow_fn)
  {
    double top = 0.;
    int sp = 0;
    /* the whole instruction at once, and the next one before this one is executed: on the device one 16-byte scalar
     * load per instruction, issued one instruction ahead of its use */
    ExprInstruction next = code[0];
    for (int i = 0; i < n; ++i) {
      const ExprInstruction ins = next;
      next = code[i + 1 < n ? i + 1 : i];
      const int op = ins.op;
      if (op <= kExVar) {
        /* slot 0 receives the unused initial `top` on the first push: depth operands take depth slots */
        stack.store(sp++, top);
        if (op == kExConst) {
          top = ins.value;
        } else {
          const int slot = ins.slot;
          top = slot == 0 ? x : (slot == 1 ? y : (slot == 2 ? z : t));
        }
      } else if (op <= kExMax) {
        const double a = stack.load(--sp);
        const double b = top;
        switch (op) {
        case kExAdd: top = a + b; break;
        case kExSub: top = a - b; break;
        case kExMul: top = a * b; break;
        case kExDiv: top = a / b; break;
        case kExPow: top = pow_fn(a, b); break;
        case kExLt: top = a < b ? 1. : 0.; break;
        case kExGt: top = a > b ? 1. : 0.; break;
        case kExLe: top = a <= b ? 1. : 0.; break;
        case kExGe: top = a >= b ? 1. : 0.; break;
        case kExEq: top = a == b ? 1. : 0.; break;
        case kExNe: top = a != b ? 1. : 0.; break;
        case kExAnd: top = (a != 0. && b != 0.) ? 1. : 0.; break;
        case kExOr: top = (a != 0. || b != 0.) ? 1. : 0.; break;
        case kExAndRounded: top = (expr_round(a) != 0. && expr_round(b) != 0.) ? 1. : 0.; break;
        case kExOrRounded: top = (expr_round(a) != 0. || expr_round(b) != 0.) ? 1. : 0.; break;
        case kExMin: top = b < a ? b : a; break; /* std::min(a, b) */
        default: top = a < b ? b : a; break;     /* kExMax: std::max(a, b) */
        }
      } else if (op <= kExSelectRounded) {
        const double a = stack.load(sp - 1);
        const double c = stack.load(sp - 2);
        sp -= 2;
        const bool taken = op == kExSelect ? c != 0. : expr_round(c) != 0.;
        top = taken ? a : top;
      } else {
        const double a = top;
        switch (op) {
        case kExNeg: top = -a; break;
        case kExPow2: top = a * a; break;
        case kExPow3: top = a * a * a; break;
        case kExPow4: top = a * a * a * a; break;
        case kExSin: top = ::sin(a); break;
        case kExCos: top = ::cos(a); break;
        case kExTan: top = ::tan(a); break;
        case kExAsin: top = ::asin(a); break;
        case kExAcos: top = ::acos(a); break;
        case kExAtan: top = ::atan(a); break;
        case kExSinh: top = ::sinh(a); break;
        case kExCosh: top = ::cosh(a); break;
        case kExTanh: top = ::tanh(a); break;
        case kExAsinh: top = ::asinh(a); break;
        case kExAcosh: top = ::acosh(a); break;
        case kExAtanh: top = ::atanh(a); break;
        case kExExp: top = ::exp(a); break;
        case kExLog: top = ::log(a); break;
        case kExLog2: top = ::log2(a); break;
        case kExLog10: top = ::log10(a); break;
        case kExSqrt: top = ::sqrt(a); break;
        case kExAbs: top = ::fabs(a); break;
        case kExSign: top = a < 0. ? -1. : (a > 0. ? 1. : 0.); break;
        case kExRint: top = ::floor(a + 0.5); break;
        case kExFloor: top = ::floor(a); break;
        case kExCeil: top = ::ceil(a); break;
        case kExInt: top = expr_round(a); break;
        case kExCot: top = 1. / ::tan(a); break;
        case kExCsc: top = 1. / ::sin(a); break;
        case kExSec: top = 1. / ::cos(a); break;
        case kExErf: top = ::erf(a); break;
        case kExErfc: top = ::erfc(a); break;
        default: /* kExResult */
          stack.store(RYUJIN_EXPR_MAX_STACK + ins.slot, a);
          sp = 0;
          break;
        }
      }
    }
    return top;
  }

  /* ---- host: the parser ---------------------------------------------------------------------------------- */

  struct ExprHostStack {
    double v[RYUJIN_EXPR_MAX_STACK];
    double load(const int slot) const { return v[slot]; }
    void store(const int slot, const double value) { v[slot] = value; }
  };

  struct ExprHostPow {
    double operator()(const double a, const double b) const { return std::pow(a, b); }
  };

  /* The variable names an expression may use, in the order of their slots. The first `n_spatial` of them are
   * coordinates: the one with index v is defined from dimension v + 1 on. */
  struct ExprVariables {
    const char *const *names;
    int n, n_spatial;
  };

  inline ExprVariables expr_variables_xyzt()
  {
    static const char *const names[4] = {"x", "y", "z", "t"};
    return ExprVariables{names, 4, 3};
  }

  /* the flux of the scalar conservation equation: the state alone (x, y, z and t are unknown identifiers) */
  inline ExprVariables expr_variables_u()
  {
    static const char *const names[1] = {"u"};
    return ExprVariables{names, 1, 0};
  }

  class ExprParser
  {
  public:
    /* the expression is text[begin, end), end = npos: up to the terminator; positions count in the whole of `text` */
    ExprParser(const char *text, const int dim, ExprProgram &program,
               const ExprVariables &variables = expr_variables_xyzt(), const size_t begin = 0,
               const size_t end = (size_t)-1)
        : s_(text)
        , len_(end == (size_t)-1 ? std::strlen(text) : end)
        , pos_(begin)
        , begin_(begin)
        , dim_(dim)
        , vars_(variables)
        , prog_(program)
    {
    }

    /* kExprOk, or the status of the refusal with `error` naming the character position (0-based) */
    int compile(std::string &error)
    {
      prog_.n = 0;
      prog_.depth = 0;
      if (dim_ < 1 || dim_ > 3)
        fail(kExprErrArg, 0, "dimension outside 1 .. 3");
      for (size_t i = begin_; i < len_ && !status_; ++i)
        if (s_[i] == '"' || s_[i] == '\'')
          fail(kExprErrUnsupported, i, "string arguments are not offered");
      skip();
      if (!status_ && pos_ == len_)
        fail(kExprErrArg, pos_, "empty expression");
      ternary();
      skip();
      if (!status_ && pos_ < len_) {
        if (s_[pos_] == '=')
          fail(kExprErrUnsupported, pos_, "assignment is not offered");
        else
          fail(kExprErrArg, pos_, s_[pos_] == ')' ? "unbalanced ')'" : "unexpected text");
      }
      if (status_) {
        error = "expression: " + message_ + " at character " + std::to_string(error_pos_) + " of \"" + s_ + "\"";
        return status_;
      }
      return kExprOk;
    }

  private:
    const char *s_;
    size_t len_, pos_, begin_;
    int dim_;
    ExprVariables vars_;
    ExprProgram &prog_;
    int live_ = 0, nesting_ = 0;
    int status_ = 0;
    size_t error_pos_ = 0;
    std::string message_;

    void fail(const int status, const size_t position, const std::string &message)
    {
      if (status_)
        return; /* the first error stands */
      status_ = status;
      error_pos_ = position;
      message_ = message;
      pos_ = len_; /* nothing is consumed after an error */
    }

    void skip()
    {
      while (pos_ < len_ && (s_[pos_] == ' ' || s_[pos_] == '\t' || s_[pos_] == '\n' || s_[pos_] == '\r'))
        ++pos_;
    }

    bool peek(const char *token)
    {
      skip();
      const size_t n = std::strlen(token);
      return !status_ && pos_ + n <= len_ && std::strncmp(s_ + pos_, token, n) == 0;
    }

    bool accept(const char *token)
    {
      if (!peek(token))
        return false;
      pos_ += std::strlen(token);
      return true;
    }

    /* `delta`: the change in the number of live operands */
    void emit(const int op, const int delta, const size_t position, const double value = 0., const int slot = 0)
    {
      if (status_)
        return;
      if (prog_.n == RYUJIN_EXPR_MAX_INSTRUCTIONS)
        return fail(kExprErrArg, position,
                    "more than " + std::to_string(RYUJIN_EXPR_MAX_INSTRUCTIONS) + " instructions");
      live_ += delta;
      if (live_ > RYUJIN_EXPR_MAX_STACK)
        return fail(kExprErrArg, position,
                    "more than " + std::to_string(RYUJIN_EXPR_MAX_STACK) + " operands alive at once");
      if (live_ > prog_.depth)
        prog_.depth = live_;
      prog_.code[prog_.n++] = ExprInstruction{op, slot, value};
    }

    struct Nested {
      ExprParser &p;
      explicit Nested(ExprParser &parser, const size_t position)
          : p(parser)
      {
        if (++p.nesting_ > kExprMaxNesting)
          p.fail(kExprErrArg, position, "nested deeper than " + std::to_string(kExprMaxNesting));
      }
      ~Nested() { --p.nesting_; }
    };

    void ternary()
    {
      logical_or();
      skip();
      const size_t at = pos_;
      if (accept("?")) {
        ternary();
        if (!accept(":"))
          return fail(kExprErrArg, pos_, "':' of '?:' expected");
        ternary();
        emit(kExSelect, -2, at);
      }
    }

    void logical_or()
    {
      logical_and();
      for (;;) {
        skip();
        const size_t at = pos_;
        if (accept("||")) {
          logical_and();
          emit(kExOr, -1, at);
        } else if (accept("|")) {
          logical_and();
          emit(kExOrRounded, -1, at);
        } else
          return;
      }
    }

    void logical_and()
    {
      comparison();
      for (;;) {
        skip();
        const size_t at = pos_;
        if (accept("&&")) {
          comparison();
          emit(kExAnd, -1, at);
        } else if (accept("&")) {
          comparison();
          emit(kExAndRounded, -1, at);
        } else
          return;
      }
    }

    void comparison()
    {
      sum();
      for (;;) {
        skip();
        const size_t at = pos_;
        int op;
        if (accept("<="))
          op = kExLe;
        else if (accept(">="))
          op = kExGe;
        else if (accept("=="))
          op = kExEq;
        else if (accept("!="))
          op = kExNe;
        else if (accept("<"))
          op = kExLt;
        else if (accept(">"))
          op = kExGt;
        else
          return;
        sum();
        emit(op, -1, at);
      }
    }

    void sum()
    {
      term();
      for (;;) {
        skip();
        const size_t at = pos_;
        if (accept("+")) {
          term();
          emit(kExAdd, -1, at);
        } else if (accept("-")) {
          term();
          emit(kExSub, -1, at);
        } else
          return;
      }
    }

    void term()
    {
      unary();
      for (;;) {
        skip();
        const size_t at = pos_;
        if (accept("*")) {
          unary();
          emit(kExMul, -1, at);
        } else if (accept("/")) {
          unary();
          emit(kExDiv, -1, at);
        } else
          return;
      }
    }

    /* sign binds weaker than ^: -x^2 = -(x^2) */
    void unary()
    {
      skip();
      const size_t at = pos_;
      if (accept("-")) {
        Nested guard(*this, at);
        unary();
        emit(kExNeg, 0, at);
      } else if (accept("+")) {
        Nested guard(*this, at);
        unary();
      } else
        power();
    }

    /* right-associative; the exponent may carry a sign: 2^-x */
    void power()
    {
      primary();
      skip();
      const size_t at = pos_;
      if (!accept("^"))
        return;
      const int before = prog_.n;
      unary();
      if (status_)
        return;
      if (prog_.n == before + 1 && prog_.code[before].op == kExConst) {
        const double e = prog_.code[before].value;
        if (e == 2. || e == 3. || e == 4.) { /* repeated multiplication instead of pow */
          --prog_.n;
          --live_;
          return emit(e == 2. ? kExPow2 : (e == 3. ? kExPow3 : kExPow4), 0, at);
        }
      }
      emit(kExPow, -1, at);
    }

    static bool is_alpha(const char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
    static bool is_digit(const char c) { return c >= '0' && c <= '9'; }

    void primary()
    {
      skip();
      if (status_)
        return;
      const size_t at = pos_;
      if (pos_ == len_)
        return fail(kExprErrArg, at, "operand expected");
      const char c = s_[pos_];
      if (c == '(') {
        Nested guard(*this, at);
        ++pos_;
        ternary();
        if (!accept(")"))
          fail(kExprErrArg, at, "unbalanced '('");
        return;
      }
      if (is_digit(c) || (c == '.' && pos_ + 1 < len_ && is_digit(s_[pos_ + 1])))
        return number();
      if (is_alpha(c))
        return identifier();
      if (c == '=')
        return fail(kExprErrUnsupported, at, "assignment is not offered");
      fail(kExprErrArg, at, "operand expected");
    }

    /* digits [. digits] [e [+-] digits] | . digits [e [+-] digits] */
    void number()
    {
      const size_t at = pos_;
      while (pos_ < len_ && is_digit(s_[pos_]))
        ++pos_;
      if (pos_ < len_ && s_[pos_] == '.') {
        ++pos_;
        while (pos_ < len_ && is_digit(s_[pos_]))
          ++pos_;
      }
      if (pos_ < len_ && (s_[pos_] == 'e' || s_[pos_] == 'E')) {
        size_t q = pos_ + 1;
        if (q < len_ && (s_[q] == '+' || s_[q] == '-'))
          ++q;
        if (q < len_ && is_digit(s_[q])) {
          while (q < len_ && is_digit(s_[q]))
            ++q;
          pos_ = q;
        }
      }
      const std::string literal(s_ + at, pos_ - at);
      emit(kExConst, +1, at, std::strtod(literal.c_str(), nullptr));
    }

    void identifier()
    {
      const size_t at = pos_;
      while (pos_ < len_ && (is_alpha(s_[pos_]) || is_digit(s_[pos_])))
        ++pos_;
      const std::string name(s_ + at, pos_ - at);
      const bool call = peek("(");

      if (name == "rand" || name == "rand_seed" || name == "sum" || name == "avg")
        return fail(kExprErrUnsupported, at, "'" + name + "' is not offered");

      if (!call) {
        for (int v = 0; v < vars_.n; ++v)
          if (name == vars_.names[v]) {
            if (v < vars_.n_spatial && v >= dim_)
              return fail(kExprErrArg, at,
                          "variable '" + name + "' is not defined in dimension " + std::to_string(dim_));
            return emit(kExVar, +1, at, 0., v);
          }
        if (name == "_pi")
          return emit(kExConst, +1, at, 3.141592653589793238462643);
        if (name == "_e")
          return emit(kExConst, +1, at, 2.718281828459045235360287);
        return fail(kExprErrArg, at, "unknown identifier '" + name + "'");
      }

      struct Unary {
        const char *name;
        int op;
      };
      static const Unary unaries[] = {
          {"sin", kExSin},     {"cos", kExCos},     {"tan", kExTan},     {"asin", kExAsin},   {"acos", kExAcos},
          {"atan", kExAtan},   {"sinh", kExSinh},   {"cosh", kExCosh},   {"tanh", kExTanh},   {"asinh", kExAsinh},
          {"acosh", kExAcosh}, {"atanh", kExAtanh}, {"exp", kExExp},     {"log", kExLog},     {"ln", kExLog},
          {"log2", kExLog2},   {"log10", kExLog10}, {"sqrt", kExSqrt},   {"abs", kExAbs},     {"sign", kExSign},
          {"rint", kExRint},   {"floor", kExFloor}, {"ceil", kExCeil},   {"int", kExInt},     {"cot", kExCot},
          {"csc", kExCsc},     {"sec", kExSec},     {"erf", kExErf},     {"erfc", kExErfc}};
      int op = -1, arity = 1; /* arity 0: one or more */
      for (const Unary &u : unaries)
        if (name == u.name)
          op = u.op;
      if (name == "pow") {
        op = kExPow;
        arity = 2;
      } else if (name == "if") {
        op = kExSelectRounded;
        arity = 3;
      } else if (name == "min" || name == "max") {
        op = name == "min" ? kExMin : kExMax;
        arity = 0;
      }
      if (op < 0)
        return fail(kExprErrArg, at, "unknown function '" + name + "'");

      Nested guard(*this, at);
      accept("(");
      int n_args = 0;
      if (!peek(")")) {
        for (;;) {
          ternary();
          ++n_args;
          if (arity == 0 && n_args > 1)
            emit(op, -1, at); /* min / max fold from the left */
          if (!accept(","))
            break;
        }
      }
      if (status_)
        return;
      if (!accept(")"))
        return fail(kExprErrArg, at, "unbalanced '(' of '" + name + "'");
      if (arity == 0 ? n_args < 1 : n_args != arity)
        return fail(kExprErrArg, at,
                    "'" + name + "' takes " + (arity == 0 ? std::string("one or more") : std::to_string(arity)) +
                        " argument(s), not " + std::to_string(n_args));
      if (arity == 1)
        emit(op, 0, at);
      else if (arity == 2)
        emit(op, -1, at);
      else if (arity == 3)
        emit(op, -2, at);
    }
  };

  /* `expression` over `variables` (by default the first `dim` of x y z, then t) -> `program`; kExprOk or the refusal
   * with its message */
  inline int expr_compile(const char *expression, const int dim, ExprProgram &program, std::string &error,
                          const ExprVariables &variables = expr_variables_xyzt())
  {
    if (!expression) {
      error = "expression: null string";
      return kExprErrArg;
    }
    return ExprParser(expression, dim, program, variables).compile(error);
  }

  /* out[i] = program(points[i * dim ..], t) with the host's library */
  inline void expr_evaluate_points(const ExprProgram &program, const int dim, const double *points, const size_t n,
                                   const double t, double *out)
  {
    ExprHostStack stack;
    for (size_t i = 0; i < n; ++i) {
      const double *p = points + i * (size_t)dim;
      out[i] = expr_evaluate(program.code, program.n, p[0], dim > 1 ? p[1] : 0., dim > 2 ? p[2] : 0., t, stack,
                             ExprHostPow{});
    }
  }

  /* ---- the flux of the scalar conservation equation: FluxLibrary "function" -------------------------------------- */

  /* source/scalar_conservation/flux_function.h: ONE string in the variable u, split at ';' into the components of the
   * flux, one per space dimension; the gradient is the central difference quotient of dealii::FunctionParser. The
   * programs of the components lie back to back, each closed by kExResult with its direction as `slot` (the layout of
   * IvFunctionProgram, initial_states_device.hpp): the same for every lane of a wave. */
  constexpr int kFluxMaxComponents = 3;

  struct FluxProgram {
    int n;              /* instructions, the kExResult closers included */
    int n_instructions; /* ... without them: what the limit RYUJIN_EXPR_MAX_INSTRUCTIONS counts, summed over the components */
    ExprInstruction code[kFluxMaxComponents * (RYUJIN_EXPR_MAX_INSTRUCTIONS + 1)];
  };

  /* `expression` in u with exactly `dim` components -> `program`; kExprOk or the refusal with its message. The limits
   * (instructions, operands, nesting) hold per component; a character position counts in the whole string. */
  inline int flux_compile(const char *expression, const int dim, FluxProgram &program, std::string &error)
  {
    program.n = 0;
    program.n_instructions = 0;
    if (!expression) {
      error = "flux: null string";
      return kExprErrArg;
    }
    if (dim < 1 || dim > kFluxMaxComponents) {
      error = "flux: dimension outside 1 .. 3";
      return kExprErrArg;
    }
    const size_t len = std::strlen(expression);
    size_t semicolon[kFluxMaxComponents] = {len, len, len}; /* the first three of them */
    int n_components = 1;
    for (size_t i = 0; i < len; ++i)
      if (expression[i] == ';') {
        if (n_components <= kFluxMaxComponents)
          semicolon[n_components - 1] = i;
        ++n_components;
      }
    if (n_components != dim) {
      const size_t at = n_components > dim ? semicolon[dim - 1] : len; /* the first ';' too many, or the end */
      error = "flux: " + std::to_string(n_components) + " component(s) separated by ';' in dimension " +
              std::to_string(dim) + " at character " + std::to_string(at) + " of \"" + expression + "\"";
      return kExprErrArg;
    }
    ExprProgram *one = new ExprProgram;
    int status = kExprOk;
    for (int d = 0; d < dim; ++d) {
      const size_t begin = d == 0 ? 0 : semicolon[d - 1] + 1;
      const size_t end = d == dim - 1 ? len : semicolon[d];
      std::string message;
      status = ExprParser(expression, dim, *one, expr_variables_u(), begin, end).compile(message);
      if (status != kExprOk) {
        error = "flux: component " + std::to_string(d) + ": " + message;
        break;
      }
      for (int i = 0; i < one->n; ++i)
        program.code[program.n++] = one->code[i];
      program.n_instructions += one->n;
      program.code[program.n++] = ExprInstruction{kExResult, d, 0.};
    }
    delete one;
    return status;
  }

  /* operands below the top one, then the values the kExResult closers leave */
  struct FluxHostStack {
    double v[RYUJIN_EXPR_MAX_STACK + kFluxMaxComponents];
    double load(const int slot) const { return v[slot]; }
    void store(const int slot, const double value) { v[slot] = value; }
  };

  /* value [n][dim] = f(u[i]) and, unless NULL, gradient [n][dim] = (f(u + delta) - f(u - delta)) / (2 * delta), in
   * the operation order of the precompute kernel (scalar_conservation_device.hpp), with the host's library */
  inline void flux_evaluate_points(const FluxProgram &program, const int dim, const double delta, const double *u,
                                   const size_t n, double *value, double *gradient)
  {
    FluxHostStack stack;
    for (size_t i = 0; i < n; ++i) {
      expr_evaluate(program.code, program.n, u[i], 0., 0., 0., stack, ExprHostPow{});
      for (int d = 0; d < dim; ++d)
        value[i * (size_t)dim + d] = stack.load(RYUJIN_EXPR_MAX_STACK + d);
      if (!gradient)
        continue;
      double plus[kFluxMaxComponents];
      expr_evaluate(program.code, program.n, u[i] + delta, 0., 0., 0., stack, ExprHostPow{});
      for (int d = 0; d < dim; ++d)
        plus[d] = stack.load(RYUJIN_EXPR_MAX_STACK + d);
      expr_evaluate(program.code, program.n, u[i] - delta, 0., 0., 0., stack, ExprHostPow{});
      for (int d = 0; d < dim; ++d)
        gradient[i * (size_t)dim + d] = (plus[d] - stack.load(RYUJIN_EXPR_MAX_STACK + d)) / (2 * delta);
    }
  }

  /* ---- the equation of state of EulerAEOS: EquationOfStateLibrary "function" -------------------------------------- */

  /* source/euler_aeos/equation_of_state_function.h: FOUR strings, pressure(rho, e), specific internal energy(rho, p),
   * temperature(rho, e) and speed of sound(rho, e). Here `e` and `p` are variables (Euler's number stays `_e`); x, y,
   * z, t and u are unknown identifiers. Slot 0 is rho, slot 1 the second variable. */
  inline ExprVariables expr_variables_rho_e()
  {
    static const char *const names[2] = {"rho", "e"};
    return ExprVariables{names, 2, 0};
  }

  inline ExprVariables expr_variables_rho_p()
  {
    static const char *const names[2] = {"rho", "p"};
    return ExprVariables{names, 2, 0};
  }

  constexpr int kEosPrograms = 4;
  enum EosFunction : int { kEosPressure = 0, kEosSpecificInternalEnergy = 1, kEosTemperature = 2, kEosSpeedOfSound = 3 };

  inline const char *eos_function_name(const int which)
  {
    static const char *const names[kEosPrograms] = {"pressure", "specific internal energy", "temperature",
                                                    "speed of sound"};
    return names[which];
  }

  /* the reference's defaults (equation_of_state_function.h:32-53): the polytropic gas with 1.4 */
  inline const char *eos_function_default(const int which)
  {
    static const char *const defaults[kEosPrograms] = {"(1.4 - 1.0) * rho * e", "p / (rho * (1.4 - 1.0))", "e / 718.",
                                                       "sqrt(1.4 * (1.4 - 1.0) * e)"};
    return defaults[which];
  }

  inline ExprVariables eos_function_variables(const int which)
  {
    return which == kEosSpecificInternalEnergy ? expr_variables_rho_p() : expr_variables_rho_e();
  }

  /* The four programs back to back, program w in code[offset[w], offset[w + 1]): a kernel runs only the one it needs,
   * whose value is what expr_evaluate returns (no kExResult closers). The same for every lane of a wave. */
  struct EosProgram {
    int offset[kEosPrograms + 1];
    int pad[3];
    ExprInstruction code[kEosPrograms * RYUJIN_EXPR_MAX_INSTRUCTIONS];
    int n_instructions(const int which) const { return offset[which + 1] - offset[which]; }
  };

  /* `expressions[w]` (NULL: the reference's default for that function) -> `program`; kExprOk or the refusal, whose
   * message names the parameter and the character position within that string. The limits (instructions, operands,
   * nesting) hold per expression. The three interpolation parameters of the surrogate must be finite. */
  inline int eos_compile(const char *const expressions[kEosPrograms], const double interpolation_b,
                         const double interpolation_pinfty, const double interpolation_q, EosProgram &program,
                         std::string &error)
  {
    for (int w = 0; w <= kEosPrograms; ++w)
      program.offset[w] = 0;
    program.pad[0] = program.pad[1] = program.pad[2] = 0;
    if (!std::isfinite(interpolation_b) || !std::isfinite(interpolation_pinfty) || !std::isfinite(interpolation_q)) {
      error = std::string("eos: interpolatory ") +
              (!std::isfinite(interpolation_b) ? "covolume b"
                                               : (!std::isfinite(interpolation_pinfty)
                                                      ? "reference pressure"
                                                      : "reference specific internal energy")) +
              " is not finite";
      return kExprErrArg;
    }
    ExprProgram *one = new ExprProgram;
    int status = kExprOk;
    for (int w = 0; w < kEosPrograms; ++w) {
      const char *text = expressions && expressions[w] ? expressions[w] : eos_function_default(w);
      std::string message;
      status = ExprParser(text, 1, *one, eos_function_variables(w)).compile(message);
      if (status != kExprOk) {
        error = std::string("eos: ") + eos_function_name(w) + ": " + message;
        break;
      }
      for (int i = 0; i < one->n; ++i)
        program.code[program.offset[w] + i] = one->code[i];
      program.offset[w + 1] = program.offset[w] + one->n;
    }
    delete one;
    return status;
  }

  /* out[i] = program `which` at (rho[i], second[i]) with the host's library; second is e, or p for the specific
   * internal energy */
  inline void eos_evaluate_points(const EosProgram &program, const int which, const double *rho, const double *second,
                                  const size_t n, double *out)
  {
    ExprHostStack stack;
    const ExprInstruction *code = program.code + program.offset[which];
    const int n_instructions = program.n_instructions(which);
    for (size_t i = 0; i < n; ++i)
      out[i] = expr_evaluate(code, n_instructions, rho[i], second[i], 0., 0., stack, ExprHostPow{});
  }
} // namespace ryujin_hip

#endif
