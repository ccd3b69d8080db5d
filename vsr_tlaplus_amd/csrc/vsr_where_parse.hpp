// vsr_where_parse.hpp — state predicates: a closed expression language over the lowered VSR.tla record, written in TLA+ syntax, compiled on the host
// into the postfix program k_where runs (vsr_where.hpp).  General TLA+ evaluation stays out of scope: this is what a user needs to ask
// "is a state with property P reachable" / "does P hold in every state" about the state variables the record stores.
//
// Input: one expression, or definitions `Name == expr`.  `\*` and `(* *)` comments.  A later definition may use an earlier name (inlined).  Every
// definition is exported (at most 8) unless it is written `LOCAL Name == expr`; a lone expression is exported under the name "where".
//
//   boolean     TRUE FALSE /\ \/ ~ => <=> ( )      precedence as in TLA+: => < <=> < /\,\/ < ~ < comparisons < .. < +,- < \div < application.
//               /\ and \/ may not be mixed without parentheses (SANY refuses that too).  No indentation-sensitive bullet lists.
//   integer     literals + - \div  ReplicaCount ClientCount StartViewOnTimerLimit Cardinality(Values)
//   comparison  = # /= < <= =< > >=  ; = and # also between statuses, message types, values, booleans and log entries (the whole record)
//   quantifier  \A x, y \in S : e   \E ...   with S = replicas | clients | Values | a..b (constant bounds) | DOMAIN rep_log[r] | DOMAIN messages
//               (at most two nested quantifiers over DOMAIN messages); x \in S with the first five as a test
//   state       rep_status[r] rep_view_number[r] rep_op_number[r] rep_commit_number[r] rep_last_normal_view[r] rep_sent_dvc[r] rep_sent_sv[r]
//               rep_peer_op_number[r][p]   rep_client_table[r][c].request_number / .op_number / .executed
//               Len(rep_log[r])   rep_log[r][i] and its fields .view_number .operation .client_id .request_number
//               Cardinality(rep_svc_recv[r])   Cardinality(rep_dvc_recv[r])
//               aux_svc   aux_client_acked[v]   v \in DOMAIN aux_client_acked
//               for m bound over DOMAIN messages: m.type .view_number .dest .source .op_number .commit_number .last_normal_vn .first_op,
//               m.message and its entry fields, messages[m] (the delivery count; keys with count 0 stay in the bag and are visited)
//   constants   Normal ViewChange Recovering, the message-type names, Nil, and — without SYMMETRY — the model values of Values
// An index may be any integer expression (rep_view_number[m.dest]): it becomes a select chain over the R (or C, or |Values|) candidates.
//
// WHERE THIS DEPARTS FROM TLC
//   * TLC raises an evaluation error for an access outside a domain.  Here such an access has a defined result: an absent log entry or message field
//     reads 0 (an absent entry's .operation equals no value and equals Nil; m.message of anything but a PrepareMsg is the absent entry);
//     aux_client_acked[v] outside its domain is FALSE; a replica or client index out of range yields -1, which equals no constant (FALSE where the
//     field is a boolean).  \div by zero gives 0.
//   * A model-value literal (v1) is refused when the model was loaded with SYMMETRY: values then enter only through bound variables, every predicate
//     is symmetric, and a hit does not depend on which member of its orbit the search stored.
//   * aux_svc and aux_client_acked are outside VIEW: of the states that differ only there the search keeps one representative (the smallest canonical
//     auxkey), and a predicate on them sees that representative.  NOT SO ON A RANDOM WALK (vsr_sim_where.hpp): a walk has
//     no VIEW representative; the aux variables a state program reads there are the walk's own — which is what TLC sees.
//   * A state of the PROBED level of the search beyond the record buffers (vsr_deep_where.hpp) has no record: it is evaluated on the
//     generated copy with the smallest key among the copies that satisfied a predicate.  Where the copies of one fingerprint differ in the aux variables
//     (an F2 tie, which the pass that inserts the level reports), that copy is one that satisfied something — not necessarily the representative the
//     level keeps when it is inserted; the scan of the inserted level one pass later sees the representative.
//
//   * (step predicates, below) the primed aux variables — aux_svc', aux_client_acked'[v] — are those of the successor AS THE ACTION GENERATES IT, before the
//     search picks the representative of its VIEW class: a pair is (stored state, generated successor), not (stored state, stored state).
//
// Refused (code 1 = VSRMC_E_ARG, message "line:col: reason"): unknown identifier, unbound variable, forward or recursive reference, type mismatch
// (rep_status[r] = 1), primes, temporal operators, CHOOSE, LAMBDA, set constructors, a quantifier over any other set, more than 8 exported names.
// Code 2 = VSRMC_E_REP: a program beyond 4096 ops or an operand depth beyond 32.
//
// THE ANALYSIS MODELS (vsrmc_predicates_compile on a model of VR_STATE_TRANSFER.tla, model_id 1, or VR_APP_STATE.tla, model_id 2).  The grammar, precedences,
// definitions, LOCAL, comments, the caps, the "line:col: reason" refusals and the SYMMETRY rule above carry over; the variable table is the spec's own
// (what depends on the model is WhereLayout below: VSR.tla's table is the same code with its own row, and compiles to the ops it always did).
//   integer     ... ReplicaCount StartViewOnTimerLimit NoProgressChangeLimit Cardinality(Values) AnyDest
//   quantifier  S = replicas | Values | a..b | DOMAIN messages | DOMAIN s for a log s | rep_recv_dvc[r] (VR_APP_STATE.tla); x \in S for all but the last two
//   state       rep_status[r] (Normal ViewChange StateTransfer) rep_view_number[r] rep_op_number[r] rep_commit_number[r] rep_last_normal_view[r]
//               rep_sent_dvc[r] rep_sent_sv[r] no_progress[r]   rep_peer_op_number[r][p]   no_progress_ctr aux_svc aux_client_acked[v] v \in DOMAIN aux_client_acked
//   logs s      rep_log[r];  m.log of a bound message — of a DoViewChangeMsg or StartViewMsg the sequence, of a NewStateMsg the function on
//               first_op..op_number, of any other type empty;  on VR_APP_STATE.tla also rep_app_state[r] and d.log of a held DoViewChange.
//               Len(s)   i \in DOMAIN s   \A / \E i \in DOMAIN s   s[i]   s[i].operation.  An entry is [operation |-> v]: s[i] = t[j] and s[i] # t[j] compare
//               entries wherever they are stored (the replica-side and message-side encodings are brought to one form by an op before anything looks at
//               them), s[i].operation is a value.  .view_number / .client_id / .request_number of an entry do not exist in these specs and are refused.
//   messages    as above: m.type .view_number .dest .source .op_number .commit_number .last_normal_vn .first_op, m.message and m.message.operation,
//               messages[m]; m.dest = AnyDest.  AnyDest equals no replica number; as an index it is out of range.
//   VR_APP_STATE.tla only   Cardinality(rep_recv_dvc[r]);  \A / \E d \in rep_recv_dvc[r] (unfolded over the source slots, guarded by the present bit: no loop;
//               r may be any integer expression) with d.type d.view_number d.source d.dest (= r) d.last_normal_vn d.op_number d.commit_number d.log.
//               On VR_STATE_TRANSFER.tla rep_app_state and rep_recv_dvc are unknown identifiers: there the DoViewChanges a replica has counted are the bag
//               keys with messages[m] = 0.
// Refused with a reason that names the model: clients ClientCount rep_client_table rep_svc_recv rep_dvc_recv Recovering; aux_restart rep_rec_number
// rep_rec_recv (never written under these cfgs: the lowering stores none of them); step_action (by the state entry: it belongs to step predicates, below).
// Refused as above by the state entry: primes, UNCHANGED, temporal operators.  A whole log as a value (m.log = rep_log[r]) is refused: compare lengths and entries.
// WHERE THIS DEPARTS FROM TLC, beyond the list above (whose conventions hold: an absent entry reads 0 and its operation equals Nil, an absent field reads 0,
// an index out of range yields -1, \div by zero gives 0):
//   * Len(m.log) is the number of entries the message carries.  For a NewStateMsg m.log is a function on first_op..op_number, not a sequence, and TLA+ gives
//     Len of it no meaning.
//   * AnyDest is an integer here (7: what m.dest reads for such a message; no replica has the number), so m.dest < AnyDest is TRUE for an addressed message
//     where TLC would refuse to compare a model value with an integer.
//
// STEP PREDICATES (where_compile(.., step = true); vsrmc_step_compile): predicates over a state and its successor — the safety half of PROPERTY, an action
// property [][P]_vars — evaluated on every transition the checker generates (vsr_step.hpp).  The same grammar plus:
//   prime        ' after a state variable name (rep_view_number'[r], rep_log'[r][i].operation, messages', aux_svc') and after a primary expression
//                (rep_view_number[r]', Len(rep_log[r])', (...)'): every state variable inside the primed expression is read in the successor; bound
//                variables and constants are what they are.  A double prime, and a prime on an expression that contains one (directly or through a
//                definition), are refused.
//   messages     \A m \in DOMAIN messages' : ... quantifies over the successor's bag, and messages'[m] is the successor's count for such an m.  At most two
//                nested message quantifiers, in any mix of bags.  A message bound over one bag as a key of the other — messages'[m] with m from DOMAIN
//                messages, m \in DOMAIN messages' as a test — would need a search of the bag and is refused.
//   UNCHANGED e  == (e' = e), for any e that can be compared with = (integers, booleans, statuses, values, log entries), for rep_log[r], and for the whole
//                per-replica variables rep_status, rep_view_number, rep_op_number, rep_commit_number, rep_last_normal_view and rep_log, where it unfolds
//                over replicas.  UNCHANGED of any other whole variable (messages, rep_client_table, ...) is refused.
//   step_action  NOT TLA+: the Next disjunct that produced the pair.  A type of its own, comparable with = / # against the fifteen action names as traces
//                print them (TimerSendSVC ReceiveHigherSVC ReceiveMatchingSVC SendDVC ReceiveHigherDVC ReceiveMatchingDVC SendSV ReceiveSV
//                ReceiveClientRequest ReceivePrepareMsg ReceivePrepareOkMsg ExecuteOp SendGetState ReceiveGetState ReceiveNewState).  TLA+ cannot name the
//                disjunct of a step; a property that needs it there restates the action's guard.
// STEP PREDICATES ON THE ANALYSIS MODELS (where_compile(.., step = true) with a model of VR_STATE_TRANSFER.tla or VR_APP_STATE.tla; vsrmc_step_predicates_compile):
// the step language above over the analysis models' variable table.
//   prime        after any state variable of the table and after a primary expression: rep_status'[r] .. rep_sent_sv'[r], no_progress'[r], no_progress_ctr',
//                rep_peer_op_number'[r][p], aux_svc', aux_client_acked'[v]; the logs rep_log'[r] and, on VR_APP_STATE.tla, rep_app_state'[r] wherever a log s may
//                stand (Len(s), DOMAIN s, s[i], s[i].operation); \A m \in DOMAIN messages', messages'[m], and m.log of a message bound over either bag (of the
//                bag it was bound over).  VR_APP_STATE.tla: Cardinality(rep_recv_dvc[r])' / Cardinality(rep_recv_dvc'[r]), \A / \E d \in rep_recv_dvc'[r]; the
//                fields and d.log of such a d are the successor's whatever the context, those of a d bound over rep_recv_dvc[r] the state's.  The rules
//                above carry over: no double prime, no prime over a prime (a bound variable cannot be primed), at most two nested message quantifiers in
//                any mix of bags, no message of one bag as a key of the other.
//   UNCHANGED e  for anything = compares; for a log of a replica, rep_log[r] or rep_app_state[r]: Len and the three positions are compared (still not a whole-log
//                value: rep_log'[r] = rep_log[r] is refused); for the whole per-replica variables rep_status, rep_view_number, rep_op_number,
//                rep_commit_number, rep_last_normal_view, rep_log, no_progress and, on VR_APP_STATE.tla, rep_app_state, unfolded over replicas.  UNCHANGED messages
//                (a bag is not a value) and UNCHANGED rep_recv_dvc (compare Cardinality, or quantify over both sets) are refused with that reason; UNCHANGED of
//                another whole variable names the list.
//   step_action  against the fifteen names of the action table (vsr_model.hpp: action_name; the three specs name their Next disjuncts alike).
// Refusals keep the "line:col: reason" form and name the model where the state language's do.  A text without primes compiles to exactly the ops
// vsrmc_predicates_compile gives it.  vsrmc_step_compile keeps refusing these models ("step predicates: VSR.tla only").
//
// Everything else keeps its meaning on both sides of a pair, the defined results of out-of-domain accesses included.  A pair whose successor equals its
// state is evaluated like any other (TLC's [][P]_vars would skip a stuttering step).  A text without primes compiles to exactly the ops the state entry
// gives it; the state entry (step = false) keeps refusing primes, UNCHANGED and step_action.  Still out of scope: temporal operators, fairness, ENABLED,
// PROPERTY / ACTION_CONSTRAINT sections of a cfg.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "vsr_where.hpp"

namespace vsr {

struct WhereProgram {
  std::vector<u32> ops;
  std::vector<std::string> names;      // exported, bit k = names[k]
  int depth = 0, msg_loops = 0, n_bodies = 0;
  bool step = false;                   // compiled by step_compile: runs over (state, successor) pairs (vsr_step.hpp), refused by k_where's entry points
};

namespace where_detail {

struct Err { int code; std::string msg; };
enum { TK_EOF, TK_ID, TK_NUM, TK_OP };
struct Tok { int kind; std::string s; long v; int line, col; };
enum { TY_INT, TY_BOOL, TY_STATUS, TY_MTYPE, TY_VALUE, TY_ENTRY, TY_ACTION };
enum { N_NUM, N_BOOL, N_ID, N_NOT, N_NEG, N_BIN, N_QUANT, N_INDEX, N_FIELD, N_CALL, N_DOMAIN, N_PRIME, N_UNCHANGED };
struct Node;
typedef std::shared_ptr<Node> NodeP;
struct Node {
  int k = 0;
  std::string s;
  long v = 0;
  int line = 0, col = 0;
  bool paren = false;
  std::vector<NodeP> c;
  std::vector<std::string> vars;
};

[[noreturn]] inline void fail_at(int line, int col, const std::string& why, int code = 1) {
  throw Err{code, std::to_string(line) + ":" + std::to_string(col) + ": " + why};
}
inline const char* type_name(int t) {
  static const char* const N[] = {"an integer", "a boolean", "a status", "a message type", "a value", "a log entry", "an action"};
  return N[t];
}

inline std::vector<Tok> lex(const std::string& t) {
  std::vector<Tok> out;
  size_t i = 0;
  int line = 1, col = 1;
  auto adv = [&](size_t n) { for (size_t k = 0; k < n && i < t.size(); k++, i++) { if (t[i] == '\n') { line++; col = 1; } else col++; } };
  static const char* const OPS[] = {"<=>", "|->", "\\/", "/\\", "=>", "==", "=<", "<=", ">=", "/=", "..", "[]", "<>", "~>", "<<", ">>", "=", "#", "<", ">",
                                    "+", "-", "~", "(", ")", "[", "]", "{", "}", ",", ":", ".", "'", "*", "|", "@", "!", "%", "&", "^", "$", "?", ";"};
  while (i < t.size()) {
    const char ch = t[i];
    if (ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n') { adv(1); continue; }
    if (t.compare(i, 2, "\\*") == 0) { while (i < t.size() && t[i] != '\n') adv(1); continue; }
    if (t.compare(i, 2, "(*") == 0) {
      const int l0 = line, c0 = col;
      int depth = 0;
      for (;;) {
        if (i >= t.size()) fail_at(l0, c0, "comment is not closed");
        if (t.compare(i, 2, "(*") == 0) { depth++; adv(2); }
        else if (t.compare(i, 2, "*)") == 0) { depth--; adv(2); if (!depth) break; }
        else adv(1);
      }
      continue;
    }
    Tok k{TK_OP, "", 0, line, col};
    if (std::isdigit((unsigned char)ch)) {
      size_t j = i;
      while (j < t.size() && std::isdigit((unsigned char)t[j])) j++;
      if (j - i > 6) fail_at(line, col, "integer literal too large");
      k.kind = TK_NUM; k.s = t.substr(i, j - i); k.v = std::stol(k.s);
      adv(j - i);
    } else if (std::isalpha((unsigned char)ch) || ch == '_') {
      size_t j = i;
      while (j < t.size() && (std::isalnum((unsigned char)t[j]) || t[j] == '_')) j++;
      k.kind = TK_ID; k.s = t.substr(i, j - i);
      adv(j - i);
    } else if (ch == '\\' && i + 1 < t.size() && std::isalpha((unsigned char)t[i + 1])) {
      size_t j = i + 1;
      while (j < t.size() && std::isalpha((unsigned char)t[j])) j++;
      k.s = t.substr(i, j - i);
      if (k.s == "\\land") k.s = "/\\";
      else if (k.s == "\\lor") k.s = "\\/";
      else if (k.s == "\\lnot" || k.s == "\\neg") k.s = "~";
      else if (k.s == "\\leq") k.s = "<=";
      else if (k.s == "\\geq") k.s = ">=";
      else if (k.s == "\\equiv") k.s = "<=>";
      adv(j - i);
    } else {
      bool found = false;
      for (const char* o : OPS) {
        const size_t n = std::strlen(o);
        if (t.compare(i, n, o) == 0) { k.s = o; adv(n); found = true; break; }
      }
      if (!found) fail_at(line, col, std::string("unexpected character '") + ch + "'");
    }
    out.push_back(k);
  }
  out.push_back(Tok{TK_EOF, "", 0, line, col});
  return out;
}

struct Parser {
  std::vector<Tok> t;
  size_t p = 0;
  bool step = false;                                            // a step predicate: ' and UNCHANGED are part of the language
  const Tok& peek(size_t a = 0) const { return t[std::min(p + a, t.size() - 1)]; }
  bool is_op(const char* s, size_t a = 0) const { return peek(a).kind == TK_OP && peek(a).s == s; }
  bool is_id(const char* s) const { return peek().kind == TK_ID && peek().s == s; }
  [[noreturn]] void fail(const Tok& k, const std::string& why) const { fail_at(k.line, k.col, why); }
  void expect(const char* s) {
    if (!is_op(s)) fail(peek(), std::string("expected '") + s + "'" + (peek().kind == TK_EOF ? " before the end of the text" : " before '" + peek().s + "'"));
    p++;
  }
  NodeP mk(int k, const Tok& at) { NodeP n = std::make_shared<Node>(); n->k = k; n->line = at.line; n->col = at.col; return n; }

  static int binprec(const Tok& k) {
    if (k.kind != TK_OP) return 0;
    const std::string& s = k.s;
    if (s == "=>") return 1;
    if (s == "<=>") return 2;
    if (s == "/\\" || s == "\\/") return 3;
    if (s == "=" || s == "#" || s == "/=" || s == "<" || s == "<=" || s == "=<" || s == ">" || s == ">=" || s == "\\in") return 5;
    if (s == "..") return 9;
    if (s == "+" || s == "-") return 10;
    if (s == "\\div") return 13;
    return 0;
  }
  void refuse_unsupported(const Tok& k) const {
    if (k.kind == TK_OP) {
      const std::string& s = k.s;
      if (s == "'" && !step) fail(k, "primed variables are not part of a state predicate");
      if (s == "[]" || s == "<>" || s == "~>") fail(k, step ? "temporal operators are not part of a step predicate" : "temporal operators are not part of a state predicate");
      if (s == "{" || s == "<<" || s == "|->" || s == "\\cup" || s == "\\cap" || s == "\\union" || s == "\\intersect" || s == "\\subseteq" || s == "\\X" || s == "\\times")
        fail(k, "set, tuple and record constructors are not supported");
      if (s == "\\notin") fail(k, "\\notin is not supported: write ~(x \\in S)");
    } else if (k.kind == TK_ID) {
      const std::string& s = k.s;
      if (s == "CHOOSE" || s == "LAMBDA") fail(k, s + " is not supported");
      if (step && s == "UNCHANGED") return;
      if (s == "ENABLED" || s == "UNCHANGED" || s == "WF_vars" || s == "SF_vars")
        fail(k, s + (step ? ": not part of a step predicate" : ": action and temporal operators are not part of a state predicate"));
      if (s == "IF" || s == "THEN" || s == "ELSE" || s == "LET" || s == "IN" || s == "CASE" || s == "SUBSET" || s == "UNION" || s == "EXCEPT") fail(k, s + " is not supported");
    }
  }

  NodeP expr(int minprec) {
    NodeP lhs = unary();
    for (;;) {
      const Tok op = peek();
      refuse_unsupported(op);
      const int pr = binprec(op);
      if (pr == 0 || pr < minprec) return lhs;
      p++;
      if (pr == 3 && lhs->k == N_BIN && !lhs->paren && (lhs->s == "/\\" || lhs->s == "\\/") && lhs->s != op.s)
        fail(op, "/\\ and \\/ are mixed without parentheses");
      NodeP rhs = op.s == "=>" ? expr(pr) : expr(pr + 1);          // => groups to the right, the others to the left
      NodeP n = mk(N_BIN, op);
      n->s = op.s == "/=" ? "#" : op.s == "=<" ? "<=" : op.s;
      n->c = {lhs, rhs};
      lhs = n;
    }
  }
  NodeP unary() {
    const Tok k = peek();
    refuse_unsupported(k);
    if (is_op("~")) { p++; NodeP n = mk(N_NOT, k); n->c = {expr(4)}; return n; }
    if (is_op("-")) { p++; NodeP n = mk(N_NEG, k); n->c = {expr(12)}; return n; }
    if (is_op("\\A") || is_op("\\E")) {
      p++;
      NodeP n = mk(N_QUANT, k);
      n->s = k.s == "\\A" ? "A" : "E";
      for (;;) {
        if (peek().kind != TK_ID) fail(peek(), "expected a variable name");
        n->vars.push_back(peek().s);
        p++;
        if (is_op(",")) { p++; continue; }
        break;
      }
      if (!is_op("\\in")) fail(peek(), "expected \\in (an unbounded quantifier cannot be evaluated)");
      p++;
      NodeP set = expr(6);
      expect(":");
      n->c = {set, expr(1)};
      return n;
    }
    if (is_id("DOMAIN")) { p++; NodeP n = mk(N_DOMAIN, k); n->c = {postfix()}; return n; }
    if (step && is_id("UNCHANGED")) { p++; NodeP n = mk(N_UNCHANGED, k); n->c = {unary()}; return n; }
    return postfix();
  }
  NodeP postfix() {
    NodeP n = primary();
    for (;;) {
      const Tok k = peek();
      if (is_op("[")) {
        p++;
        NodeP ix = mk(N_INDEX, k);
        ix->c = {n, expr(1)};
        expect("]");
        n = ix;
      } else if (is_op(".")) {
        p++;
        if (peek().kind != TK_ID) fail(peek(), "expected a field name");
        NodeP f = mk(N_FIELD, peek());
        f->s = peek().s;
        f->c = {n};
        p++;
        n = f;
      } else if (is_op("'")) {
        refuse_unsupported(k);
        if (n->k == N_PRIME) fail(k, "double prime");
        p++;
        NodeP pr = mk(N_PRIME, k);
        pr->c = {n};
        n = pr;
      } else {
        return n;
      }
    }
  }
  NodeP primary() {
    const Tok k = peek();
    refuse_unsupported(k);
    if (k.kind == TK_NUM) { p++; NodeP n = mk(N_NUM, k); n->v = k.v; return n; }
    if (k.kind == TK_ID) {
      p++;
      if (k.s == "TRUE" || k.s == "FALSE") { NodeP n = mk(N_BOOL, k); n->v = k.s == "TRUE"; return n; }
      if (is_op("(")) {
        if (k.s != "Cardinality" && k.s != "Len") fail(k, "unknown operator " + k.s + " (Cardinality and Len are the operators that take an argument)");
        p++;
        NodeP n = mk(N_CALL, k);
        n->s = k.s;
        n->c = {expr(1)};
        expect(")");
        return n;
      }
      NodeP n = mk(N_ID, k);
      n->s = k.s;
      return n;
    }
    if (is_op("(")) { p++; NodeP n = expr(1); expect(")"); n->paren = true; return n; }
    if (is_op("[")) fail(k, "function and record constructors are not supported");
    fail(k, k.kind == TK_EOF ? "expression expected before the end of the text" : "expression expected before '" + k.s + "'");
  }
};

// kind 0: integer constant, 1: value constant (index + 1), 2: message loop v (primed: over messages'), 3: a held DoViewChange, v = replica << 4 | source slot
// (primed: of rep_recv_dvc'[r] — its fields are read in the successor whatever the context)
struct Binding { std::string name; int kind; int v; bool primed = false; };
struct Def { NodeP body; };

// What depends on the model: where a variable lies in the record and which names exist (vsr_model.hpp, vrst_actions.hpp, vras_actions.hpp).  Shared by the
// three and therefore not here: the header (aux_svc, aux_client_acked), the A word's first 14 bits (status .. rep_sent_sv), the bag word, and the A word of
// replica r at 1 + (r - 1) * Model::wpr.
struct WhereLayout {
  const char* spec;        // the module, for messages
  bool analysis;           // an analysis model: an entry is [operation |-> v], statuses Normal / ViewChange / StateTransfer, AnyDest, no clients
  int peer_shift;          // rep_peer_op_number[r][p]: 2 bits at peer_shift + 2 (p - 1) of the A word
  int noprog_shift;        // no_progress[r] in the A word, no_progress_ctr at bit 20 of the header; -1: the model has neither
  int log_word, log_shift, log_width;   // rep_log[r]: in word aword(r) + log_word; 24 bits of entry bytes, or 9 bits of 3-bit entries
  bool app_state;          // rep_app_state (A word, from bit 34) and rep_recv_dvc (the B word) exist
};
inline const WhereLayout& where_layout(int model_id) {
  static const WhereLayout Y[3] = {{"VSR.tla", false, 19, -1, 1, 0, 24, false},
                                   {"VR_STATE_TRANSFER.tla", true, 15, 14, 0, 25, 9, false},
                                   {"VR_APP_STATE.tla", true, 15, 14, 0, 25, 9, true}};
  return Y[model_id >= 0 && model_id <= 2 ? model_id : 0];
}

struct Compiler {
  const Model& M;
  bool symmetry;
  const std::vector<std::string>& values;
  WhereProgram& out;
  std::vector<Binding> env;
  std::map<std::string, Def> defs;
  std::string compiling;                                      // the definition being compiled (recursion)
  int cur = 0, msg_depth = 0;
  bool step = false;                                          // a step predicate: step_action and the action names exist
  bool P = false;                                             // the loads being emitted read the successor (inside a primed expression)
  const WhereLayout& Y;
  const bool AN;                                              // an analysis model

  Compiler(const Model& m, bool sym, const std::vector<std::string>& vals, WhereProgram& o)
      : M(m), symmetry(sym), values(vals), out(o), Y(where_layout(m.model_id)), AN(Y.analysis) {}

  void emit(int code, u32 arg, int delta) {
    if (out.ops.size() + 1 >= (size_t)WHERE_MAX_OPS) throw Err{2, "state predicates: the program has more than " + std::to_string((int)WHERE_MAX_OPS) + " ops"};
    out.ops.push_back(w_op(code, arg));
    cur += delta;
    if (cur > out.depth) out.depth = cur;
    if (cur > (int)WHERE_MAX_DEPTH) throw Err{2, "state predicates: operand depth beyond " + std::to_string((int)WHERE_MAX_DEPTH)};
  }
  void push(int v) { emit(W_PUSH, (u32)v & 0xFFFFFFu, +1); }
  void ldbits(int word, int shift, int width) { emit(W_LDBITS, (u32)word | ((u32)shift << 8) | ((u32)width << 14) | ((u32)P << 20), +1); }
  void ldm(int loop, int shift, int width) { emit(W_LDM, (u32)loop | ((u32)shift << 1) | ((u32)width << 7), +1); }
  void bin(int code) { emit(code, 0, -1); }
  int aword(int r) const { return 1 + (r - 1) * M.wpr; }

  const Binding* lookup(const std::string& s) const {
    for (size_t i = env.size(); i-- > 0;)
      if (env[i].name == s) return &env[i];
    return nullptr;
  }
  [[noreturn]] void fail(const NodeP& n, const std::string& why) const { fail_at(n->line, n->col, why); }
  void want(const NodeP& n, int got, int need) const {
    if (got != need) fail(n, std::string("type mismatch: ") + type_name(need) + " is needed here, this is " + type_name(got));
  }
  int value_literal(const std::string& s) const {
    for (size_t v = 0; v < values.size(); v++)
      if (values[v] == s) return (int)v + 1;
    return 0;
  }

  // compile-time integers: literals, the model's constants, bound variables of unfolded quantifiers, + - \div of those
  bool const_int(const NodeP& n, int* v) const {
    switch (n->k) {
      case N_NUM: *v = (int)n->v; return true;
      case N_NEG: { int a; if (!const_int(n->c[0], &a)) return false; *v = -a; return true; }
      case N_ID: {
        if (const Binding* b = lookup(n->s)) { if (b->kind != 0) return false; *v = b->v; return true; }
        if (n->s == "ReplicaCount") { *v = M.R; return true; }
        if (n->s == "ClientCount" && !AN) { *v = M.C; return true; }
        if (n->s == "NoProgressChangeLimit" && AN) { *v = 0; return true; }                 // (the lowering accepts no other value)
        if (n->s == "StartViewOnTimerLimit") { *v = M.L; return true; }
        return false;
      }
      case N_CALL:
        if (n->s == "Cardinality" && n->c[0]->k == N_ID && n->c[0]->s == "Values" && !lookup("Values")) { *v = M.n; return true; }
        return false;
      case N_BIN: {
        int a, b;
        if (n->s != "+" && n->s != "-" && n->s != "\\div") return false;
        if (!const_int(n->c[0], &a) || !const_int(n->c[1], &b)) return false;
        if (n->s == "+") *v = a + b;
        else if (n->s == "-") *v = a - b;
        else { *v = 0; if (b) { *v = a / b; if ((a % b) && ((a < 0) != (b < 0))) (*v)--; } }
        return true;
      }
    }
    return false;
  }
  bool const_value(const NodeP& n, int* v) const {
    if (n->k != N_ID) return false;
    if (const Binding* b = lookup(n->s)) { if (b->kind != 1) return false; *v = b->v; return true; }
    if (!symmetry && value_literal(n->s)) { *v = value_literal(n->s); return true; }
    return false;
  }

  // f[i1][i2]..: every index is a constant, or becomes a select chain over its candidates lo..hi.  `leaf` emits the load for one tuple of constants.
  struct Ix { NodeP n; int lo, hi, type; };
  // lp: the leaf loads read the successor (f'[i]: the variable is primed, the index expressions are whatever the context is)
  void indexed(const std::vector<Ix>& ixs, size_t at, std::vector<int>& vals, int deflt, const std::function<void(const std::vector<int>&)>& leaf, bool lp) {
    if (at == ixs.size()) { const bool saved = P; P = lp; leaf(vals); P = saved; return; }
    const Ix& x = ixs[at];
    int v;
    if (x.type == TY_INT ? const_int(x.n, &v) : const_value(x.n, &v)) {
      if (v < x.lo || v > x.hi) { push(deflt); return; }
      vals.push_back(v);
      indexed(ixs, at + 1, vals, deflt, leaf, lp);
      vals.pop_back();
      return;
    }
    push(deflt);
    for (int k = x.lo; k <= x.hi; k++) {
      want(x.n, compile(x.n), x.type);
      push(k);
      bin(W_EQ);
      vals.push_back(k);
      indexed(ixs, at + 1, vals, deflt, leaf, lp);
      vals.pop_back();
      emit(W_SEL, 0, -2);
    }
  }

  // n = root[..][..].field... : the accessors from the root outwards
  struct Acc { bool field; std::string name; NodeP ix; NodeP at; };
  NodeP flatten(NodeP n, std::vector<Acc>& acc) const {
    while (n->k == N_INDEX || n->k == N_FIELD) {
      acc.insert(acc.begin(), n->k == N_INDEX ? Acc{false, "", n->c[1], n} : Acc{true, n->s, nullptr, n});
      n = n->c[0];
    }
    return n;
  }
  // v' with v a state variable: the bare name, *primed set.  (A prime further out is the context's P.)
  NodeP strip_prime(NodeP root, bool* primed) const {
    *primed = false;
    if (root->k == N_PRIME && root->c[0]->k == N_ID && !lookup(root->c[0]->s) && !defs.count(root->c[0]->s)) {
      if (P) fail(root, "double prime: " + root->c[0]->s + "' inside an expression that is primed");
      *primed = true;
      return root->c[0];
    }
    return root;
  }
  static bool has_prime(const NodeP& n) {
    if (n->k == N_PRIME || n->k == N_UNCHANGED) return true;
    for (const NodeP& c : n->c)
      if (has_prime(c)) return true;
    return false;
  }
  int entry_field(const NodeP& at, const std::string& f) {
    if (AN) {                                                   // the entry is already its value + 1
      if (f == "operation") return TY_VALUE;
      if (f == "view_number" || f == "client_id" || f == "request_number")
        fail(at, std::string("a log entry of ") + Y.spec + " is [operation |-> v]: it has no field " + f);
      fail(at, "a log entry has no field " + f + " (operation)");
    }
    const int k = f == "view_number" ? 0 : f == "operation" ? 1 : f == "client_id" ? 2 : f == "request_number" ? 3 : -1;
    if (k < 0) fail(at, "a log entry has no field " + f + " (view_number, operation, client_id, request_number)");
    emit(W_ENTF, (u32)k, 0);
    return k == 1 ? TY_VALUE : TY_INT;
  }
  void emit_log_len(const NodeP& r, bool lp) {                 // Len(rep_log[r])
    std::vector<int> vals;
    indexed({Ix{r, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& v) { ldbits(aword(v[0]) + Y.log_word, Y.log_shift, Y.log_width); emit(W_LOGLEN, 0, 0); }, lp);
  }
  // rep_log[r] / rep_log'[r] as the argument of Len / DOMAIN: returns the index node r; *lp = the log is the successor's
  NodeP log_of(const NodeP& n, bool* lp) const {
    if (AN) return nullptr;                                     // (seq_of, below)
    std::vector<Acc> acc;
    bool pr = false;
    NodeP root = flatten(n, acc);
    if (root->k == N_PRIME && root->c[0]->k == N_ID && root->c[0]->s == "rep_log") root = strip_prime(root, &pr);
    *lp = P || pr;
    if (root->k == N_ID && root->s == "rep_log" && !lookup("rep_log") && acc.size() == 1 && !acc[0].field) return acc[0].ix;
    return nullptr;
  }

  // ---- the analysis models ----------------------------------------------------------------------------------------------------------------------
  // names the spec has (or VSR.tla has) but this model's lowering does not
  void refuse_absent(const NodeP& at, const std::string& s) const {
    if (!AN) return;
    if (s == "clients" || s == "ClientCount" || s == "rep_client_table")
      fail(at, s + ": " + Y.spec + " has no clients (a request is ReceiveClientRequest(r, v) for a value v)");
    if (s == "rep_svc_recv" || s == "rep_dvc_recv")
      fail(at, s + " is not a variable of " + Y.spec + (Y.app_state ? ": the DoViewChanges a replica holds are rep_recv_dvc[r]"
                                                                     : ": the messages a replica has counted are the bag keys with messages[m] = 0"));
    if (s == "Recovering") fail(at, std::string("Recovering is not a status of ") + Y.spec + " (Normal, ViewChange, StateTransfer)");
    if (s == "aux_restart" || s == "rep_rec_number" || s == "rep_rec_recv" || s == "RecoveryMsg" || s == "RecoveryResponseMsg")
      fail(at, s + " is never written under the cfg of " + Y.spec + ": the lowering does not store it");
    if (s == "step_action" && !step) fail(at, std::string("step_action belongs to step predicates, which are not built for ") + Y.spec);
  }
  // a sequence of entries: 1 rep_log[r], 2 rep_app_state[r], 3 m.log of a bound message, 4 d.log of a held DoViewChange
  // lp: the sequence is the successor's (rep_log'[r], or the context is primed; d.log of a d bound over rep_recv_dvc'[r]); m.log is the loop's bag word
  struct Seq { int kind = 0; NodeP r; int loop = 0, dr = 0, ds = 0; bool lp = false; };
  bool seq_of(const NodeP& n, Seq* q) const {
    std::vector<Acc> acc;
    bool pr = false;
    NodeP root = flatten(n, acc);
    if (root->k == N_PRIME && root->c[0]->k == N_ID && (root->c[0]->s == "rep_log" || (Y.app_state && root->c[0]->s == "rep_app_state"))) root = strip_prime(root, &pr);
    if (root->k != N_ID || acc.size() != 1) return false;
    if (const Binding* b = lookup(root->s)) {
      if (!acc[0].field || acc[0].name != "log") return false;
      if (b->kind == 2) { q->kind = 3; q->loop = b->v; return true; }
      if (b->kind == 3) { q->kind = 4; q->dr = b->v >> 4; q->ds = b->v & 15; q->lp = b->primed; return true; }
      return false;
    }
    if (acc[0].field || defs.count(root->s)) return false;
    q->r = acc[0].ix;
    q->lp = P || pr;
    if (root->s == "rep_log") { q->kind = 1; return true; }
    if (Y.app_state && root->s == "rep_app_state") { q->kind = 2; return true; }
    return false;
  }
  int bword(int r) const { return aword(r) + 1; }              // rep_recv_dvc[r] (vras_actions.hpp)
  static int dvc_shift(int s) { return 3 + 17 * (s - 1); }
  void seq_len(const Seq& q) {
    std::vector<int> vals;
    switch (q.kind) {
      case 1: indexed({Ix{q.r, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& v) { ldbits(aword(v[0]) + Y.log_word, Y.log_shift, Y.log_width); emit(W_BLOGLEN, 0, 0); }, q.lp); break;
      case 2: indexed({Ix{q.r, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& v) { ldbits(aword(v[0]), 7, 2); }, q.lp); break;   // Len(rep_app_state[r]) = rep_commit_number[r]
      case 3: emit(W_MLOGLEN, (u32)q.loop, +1); break;
      case 4: indexed({}, 0, vals, 0, [&](const std::vector<int>&) { ldbits(bword(q.dr), dvc_shift(q.ds) + 8, 9); emit(W_BLOGLEN, 0, 0); }, q.lp); break;
    }
  }
  // entry i of the sequence in the one form every entry is compared in (value + 1, 0 = absent: outside the domain, or a replica out of range)
  void seq_entry(const Seq& q, const NodeP& i) {
    std::vector<int> vals;
    switch (q.kind) {
      case 1:
        indexed({Ix{q.r, 1, M.R, TY_INT}, Ix{i, 1, 3, TY_INT}}, 0, vals, 0,
                [&](const std::vector<int>& v) { ldbits(aword(v[0]) + Y.log_word, Y.log_shift + 3 * (v[1] - 1), 3); emit(W_ENTN, 0, 0); }, q.lp);
        break;
      case 2:
        indexed({Ix{q.r, 1, M.R, TY_INT}, Ix{i, 1, 3, TY_INT}}, 0, vals, 0,
                [&](const std::vector<int>& v) { emit(W_APPENT, (u32)aword(v[0]) | ((u32)v[1] << 8) | ((u32)P << 20), +1); }, q.lp);
        break;
      case 3: indexed({Ix{i, 1, 3, TY_INT}}, 0, vals, 0, [&](const std::vector<int>& v) { emit(W_MLOGENT, (u32)q.loop | ((u32)v[0] << 1), +1); }, false); break;
      case 4:
        indexed({Ix{i, 1, 3, TY_INT}}, 0, vals, 0,
                [&](const std::vector<int>& v) { ldbits(bword(q.dr), dvc_shift(q.ds) + 8 + 3 * (v[0] - 1), 3); emit(W_ENTN, 0, 0); }, q.lp);
        break;
    }
  }
  // x.log... with x a bound message or held DoViewChange: acc[0] is the field `log`
  int compile_log_path(const NodeP& n, const std::vector<Acc>& acc, const Seq& q) {
    if (acc.size() == 1)
      fail(acc[0].at, "a whole log cannot be compared or used as a value: Len(x.log), x.log[i], x.log[i].operation, i \\in DOMAIN x.log and a quantifier over DOMAIN x.log are the supported forms");
    if (acc[1].field || acc.size() > 3 || (acc.size() == 3 && !acc[2].field)) fail(n, "x.log[i] and x.log[i].operation are the supported forms");
    seq_entry(q, acc[1].ix);
    return acc.size() == 3 ? entry_field(acc[2].at, acc[2].name) : TY_ENTRY;
  }
  // \A / \E d \in rep_recv_dvc[r]: unfolded over the source slots, each guarded by its present bit; a replica that is not a constant unfolds over replicas too
  // lp: the set is the successor's (rep_recv_dvc'[r], or the context is primed)
  void quant_dvc(const NodeP& n, size_t var, const NodeP& r, bool lp) {
    const bool forall = n->s == "A";
    auto slots = [&](int rv) {
      for (int s = 1; s <= M.R; s++) {
        { const bool saved = P; P = lp; ldbits(bword(rv), dvc_shift(s), 1); P = saved; }
        env.push_back(Binding{n->vars[var], 3, (rv << 4) | s, lp});
        compile_quant(n, var + 1);
        env.pop_back();
        bin(forall ? W_IMP : W_AND);
        if (s > 1) bin(forall ? W_AND : W_OR);
      }
    };
    int rv;
    if (const_int(r, &rv)) {
      if (rv < 1 || rv > M.R) push(forall); else slots(rv);    // a replica out of range holds nothing
      return;
    }
    for (rv = 1; rv <= M.R; rv++) {
      want(r, compile(r), TY_INT);
      push(rv);
      bin(W_EQ);
      slots(rv);
      bin(forall ? W_IMP : W_AND);
      if (rv > 1) bin(forall ? W_AND : W_OR);
    }
  }

  int compile_path(const NodeP& n) {
    std::vector<Acc> acc;
    bool root_primed = false;
    NodeP root = strip_prime(flatten(n, acc), &root_primed);
    if (root->k == N_PRIME && root->c[0]->k == N_ID && lookup(root->c[0]->s)) fail(root, root->c[0]->s + " is a bound variable: it cannot be primed");
    if (root->k == N_PRIME && has_prime(root->c[0])) fail(root, "double prime: a primed expression that is indexed is primed again");
    if (root->k != N_ID) fail(n, "only state variables and bound messages can be indexed or have fields");
    const bool lp = P || root_primed;
    const std::string& s = root->s;
    auto shape = [&](std::initializer_list<bool> fields) {     // the accessors must be exactly: index (false) / field (true) in this order
      if (acc.size() != fields.size()) return false;
      size_t i = 0;
      for (bool f : fields) if (acc[i++].field != f) return false;
      return true;
    };
    std::vector<int> vals;
    if (const Binding* b = lookup(s)) {
      if (root_primed) fail(n, s + " is a bound variable: it cannot be primed");
      if (b->kind == 3) {                                       // a held DoViewChange of rep_recv_dvc[dr], from source ds
        const int dr = b->v >> 4, ds = b->v & 15;
        if (!acc[0].field) fail(acc[0].at, "a message cannot be indexed");
        const std::string& f = acc[0].name;
        if (f == "log") { Seq q; q.kind = 4; q.dr = dr; q.ds = ds; q.lp = b->primed; return compile_log_path(n, acc, q); }
        if (acc.size() != 1) fail(n, s + "." + f + " has no fields and cannot be indexed");
        if (f == "type") { push(T_DVC); return TY_MTYPE; }
        if (f == "source") { push(ds); return TY_INT; }
        if (f == "dest") { push(dr); return TY_INT; }
        static const struct { const char* name; int shift, width; } DF[] = {{"view_number", -1, 3}, {"last_normal_vn", 1, 3}, {"op_number", 4, 2}, {"commit_number", 6, 2}};
        for (const auto& e : DF)
          if (f == e.name) {                                    // of the side d was bound on, whatever the context
            const bool saved = P;
            P = b->primed;
            ldbits(bword(dr), e.shift < 0 ? 0 : dvc_shift(ds) + e.shift, e.width);
            P = saved;
            return TY_INT;
          }
        fail(acc[0].at, "a DoViewChangeMsg has no field " + f);
      }
      if (b->kind != 2) fail(n, s + " is not a message: it has no fields and cannot be indexed");
      const int d = b->v;
      if (!acc[0].field) fail(acc[0].at, "a message cannot be indexed");
      const std::string& f = acc[0].name;
      if (AN && f == "log") { Seq q; q.kind = 3; q.loop = d; return compile_log_path(n, acc, q); }
      if (f == "message") {
        emit(W_LDMENT, (u32)d, +1);
        if (AN) emit(W_ENTN, 1, 0);
        if (acc.size() == 1) return TY_ENTRY;
        if (acc.size() == 2 && acc[1].field) return entry_field(acc[1].at, acc[1].name);
        fail(n, "m.message is a log entry: one field at most");
      }
      if (acc.size() != 1) fail(n, "m." + f + " has no fields and cannot be indexed");
      if (f == "type") { ldm(d, 0, 3); return TY_MTYPE; }
      static const struct { const char* name; int shift, width; } F[] = {{"view_number", 3, 3}, {"dest", 6, 3}, {"source", 9, 3}, {"op_number", 12, 2},
                                                                          {"commit_number", 14, 2}, {"last_normal_vn", 16, 3}, {"first_op", 19, 2}};
      for (const auto& e : F)
        if (f == e.name) { ldm(d, e.shift, e.width); return TY_INT; }
      if (f == "log") fail(acc[0].at, "m.log is not supported");
      fail(acc[0].at, "a message has no field " + f);
    }
    if (defs.count(s)) fail(n, s + " is a definition: it has no fields and cannot be indexed");
    refuse_absent(root, s);
    if (s == "messages") {
      if (!shape({false})) fail(n, "messages[m] with m bound over DOMAIN messages is the supported form");
      const Binding* b = acc[0].ix->k == N_ID ? lookup(acc[0].ix->s) : nullptr;
      if (!b || b->kind != 2) fail(acc[0].ix, "messages[m]: m must be a variable bound over DOMAIN messages");
      if (b->primed != lp)
        fail(acc[0].ix, lp ? "messages'[" + b->name + "]: " + b->name + " is bound over DOMAIN messages, not DOMAIN messages' (a lookup in the other bag is not supported)"
                           : "messages[" + b->name + "]: " + b->name + " is bound over DOMAIN messages', not DOMAIN messages (a lookup in the other bag is not supported)");
      ldm(b->v, 21, 2);
      return TY_INT;
    }
    static const struct { const char* name; int shift, width, type; } A[] = {
        {"rep_status", 0, 2, TY_STATUS}, {"rep_view_number", 2, 3, TY_INT}, {"rep_op_number", 5, 2, TY_INT}, {"rep_commit_number", 7, 2, TY_INT},
        {"rep_last_normal_view", 9, 3, TY_INT}, {"rep_sent_dvc", 12, 1, TY_BOOL}, {"rep_sent_sv", 13, 1, TY_BOOL}};
    for (const auto& e : A)
      if (s == e.name) {
        if (!shape({false})) fail(n, s + "[r] is the supported form");
        indexed({Ix{acc[0].ix, 1, M.R, TY_INT}}, 0, vals, e.type == TY_BOOL ? 0 : -1, [&](const std::vector<int>& v) { ldbits(aword(v[0]), e.shift, e.width); }, lp);
        return e.type;
      }
    if (s == "no_progress" && Y.noprog_shift >= 0) {
      if (!shape({false})) fail(n, s + "[r] is the supported form");
      indexed({Ix{acc[0].ix, 1, M.R, TY_INT}}, 0, vals, 0, [&](const std::vector<int>& v) { ldbits(aword(v[0]), Y.noprog_shift, 1); }, lp);
      return TY_BOOL;
    }
    if (s == "rep_peer_op_number") {
      if (!shape({false, false})) fail(n, "rep_peer_op_number[r][p] is the supported form");
      indexed({Ix{acc[0].ix, 1, M.R, TY_INT}, Ix{acc[1].ix, 1, M.R, TY_INT}}, 0, vals, -1,
              [&](const std::vector<int>& v) { ldbits(aword(v[0]), Y.peer_shift + 2 * (v[1] - 1), 2); }, lp);
      return TY_INT;
    }
    if (AN && (s == "rep_log" || (Y.app_state && s == "rep_app_state"))) {
      if (!shape({false, false}) && !shape({false, false, true}))
        fail(n, s + "[r][i], its .operation, Len(" + s + "[r]) and DOMAIN " + s + "[r] are the supported forms");
      Seq q;
      q.kind = s == "rep_log" ? 1 : 2;
      q.r = acc[0].ix;
      q.lp = lp;
      seq_entry(q, acc[1].ix);
      return acc.size() == 3 ? entry_field(acc[2].at, acc[2].name) : TY_ENTRY;
    }
    if (Y.app_state && s == "rep_recv_dvc") fail(n, "rep_recv_dvc: Cardinality(rep_recv_dvc[r]) and \\A / \\E d \\in rep_recv_dvc[r] are the supported forms");
    if (s == "rep_client_table") {
      if (!shape({false, false, true})) fail(n, "rep_client_table[r][c].request_number / .op_number / .executed are the supported forms");
      const std::string& f = acc[2].name;
      const int off = f == "request_number" ? 0 : f == "op_number" ? 2 : f == "executed" ? 4 : -1;
      if (off < 0) fail(acc[2].at, "a client-table row has no field " + f);
      indexed({Ix{acc[0].ix, 1, M.R, TY_INT}, Ix{acc[1].ix, 1, M.C, TY_INT}}, 0, vals, off == 4 ? 0 : -1,
              [&](const std::vector<int>& v) { ldbits(aword(v[0]), 29 + 5 * (v[1] - 1) + off, off == 4 ? 1 : 2); }, lp);
      return off == 4 ? TY_BOOL : TY_INT;
    }
    if (s == "rep_log") {
      if (!shape({false, false}) && !shape({false, false, true})) fail(n, "rep_log[r][i], its fields, Len(rep_log[r]) and DOMAIN rep_log[r] are the supported forms");
      indexed({Ix{acc[0].ix, 1, M.R, TY_INT}, Ix{acc[1].ix, 1, 3, TY_INT}}, 0, vals, 0,      // outside the log: the absent entry
              [&](const std::vector<int>& v) { ldbits(aword(v[0]) + Y.log_word, Y.log_shift + 8 * (v[1] - 1), 8); }, lp);
      return acc.size() == 3 ? entry_field(acc[2].at, acc[2].name) : TY_ENTRY;
    }
    if (s == "aux_client_acked") {
      if (!shape({false})) fail(n, "aux_client_acked[v] is the supported form");
      indexed({Ix{acc[0].ix, 1, M.n, TY_VALUE}}, 0, vals, 0, [&](const std::vector<int>& v) { ldbits(0, 11 + 2 * (v[0] - 1), 2); push(2); bin(W_EQ); }, lp);
      return TY_BOOL;
    }
    if (s == "rep_svc_recv" || s == "rep_dvc_recv") fail(n, s + ": only Cardinality(" + s + "[r]) is supported");
    compile(root);                                            // unknown identifier / not indexable: the error names it
    fail(n, s + " has no fields and cannot be indexed");
  }

  // the members lo..hi of a constant set; false = not such a set
  bool const_set(const NodeP& s, int* lo, int* hi, int* kind) {
    *kind = 0;
    if (s->k == N_ID && !lookup(s->s) && !defs.count(s->s)) {
      refuse_absent(s, s->s);
      if (s->s == "replicas") { *lo = 1; *hi = M.R; return true; }
      if (s->s == "clients") { *lo = 1; *hi = M.C; return true; }
      if (s->s == "Values") { *lo = 1; *hi = M.n; *kind = 1; return true; }
    }
    if (s->k == N_BIN && s->s == "..") {
      if (!const_int(s->c[0], lo) || !const_int(s->c[1], hi)) fail(s, "the bounds of a range must be constants");
      if (*hi - *lo > 64) fail(s, "range too large to unfold");
      return true;
    }
    return false;
  }

  int compile_quant(const NodeP& n, size_t var) {
    const NodeP& set = n->c[0];
    const bool forall = n->s == "A";
    if (var == n->vars.size()) { want(n->c[1], compile(n->c[1]), TY_BOOL); out.n_bodies++; return TY_BOOL; }
    const std::string& name = n->vars[var];
    int lo, hi, kind;
    NodeP logr;
    bool loglp = false;
    if (const_set(set, &lo, &hi, &kind)) {
      if (lo > hi) { push(forall); return TY_BOOL; }
      for (int k = lo; k <= hi; k++) {
        env.push_back(Binding{name, kind, k});
        compile_quant(n, var + 1);
        env.pop_back();
        if (k > lo) bin(forall ? W_AND : W_OR);
      }
      return TY_BOOL;
    }
    Seq q;
    if (AN && set->k == N_DOMAIN && seq_of(set->c[0], &q)) {          // the domain of a sequence: unfolded over the three positions, each guarded by its presence
      for (int k = 1; k <= 3; k++) {
        NodeP kn = std::make_shared<Node>();
        kn->k = N_NUM; kn->v = k; kn->line = set->line; kn->col = set->col;
        seq_entry(q, kn);
        push(0);
        bin(W_NE);
        env.push_back(Binding{name, 0, k});
        compile_quant(n, var + 1);
        env.pop_back();
        bin(forall ? W_IMP : W_AND);
        if (k > 1) bin(forall ? W_AND : W_OR);
      }
      return TY_BOOL;
    }
    if (Y.app_state && set->k == N_INDEX && !lookup("rep_recv_dvc") && !defs.count("rep_recv_dvc")) {
      bool hp = false;
      const NodeP held = strip_prime(set->c[0], &hp);           // rep_recv_dvc'[r]: the successor's set
      if (held->k == N_ID && held->s == "rep_recv_dvc") {
        quant_dvc(n, var, set->c[1], P || hp);
        return TY_BOOL;
      }
    }
    if (set->k == N_DOMAIN && (logr = log_of(set->c[0], &loglp))) {    // 1..Len(rep_log[r]): unfolded over the three positions, each guarded by its presence
      for (int k = 1; k <= 3; k++) {
        push(k);
        emit_log_len(logr, loglp);
        bin(W_LE);
        env.push_back(Binding{name, 0, k});
        compile_quant(n, var + 1);
        env.pop_back();
        bin(forall ? W_IMP : W_AND);
        if (k > 1) bin(forall ? W_AND : W_OR);
      }
      return TY_BOOL;
    }
    bool bagp = false;
    const NodeP bag = set->k == N_DOMAIN ? strip_prime(set->c[0], &bagp) : nullptr;
    if (bag && bag->k == N_ID && bag->s == "messages" && !lookup("messages")) {
      if (msg_depth >= 2) fail(n, "at most two nested quantifiers over DOMAIN messages");
      const bool pr = P || bagp;                                  // DOMAIN messages': the successor's bag
      const int d = msg_depth++;
      if (msg_depth > out.msg_loops) out.msg_loops = msg_depth;
      const size_t begin = out.ops.size();
      emit(W_MBEGIN, 0, 0);
      env.push_back(Binding{name, 2, d, pr});
      compile_quant(n, var + 1);
      env.pop_back();
      out.ops[begin] = w_op(W_MBEGIN, (u32)out.ops.size() | ((u32)d << 12) | ((u32)forall << 13) | ((u32)pr << 14));
      emit(W_MEND, (u32)d | ((u32)forall << 1) | ((u32)(begin + 1) << 2) | ((u32)pr << 14), 0);
      msg_depth--;
      return TY_BOOL;
    }
    if (AN) {
      const NodeP inner = set->k == N_DOMAIN ? set->c[0] : set;
      if (inner->k == N_INDEX || inner->k == N_FIELD) compile(inner);   // (an unknown or refused name says so itself)
      fail(set, std::string("a quantifier ranges over replicas, Values, a..b, DOMAIN messages, DOMAIN rep_log[r], DOMAIN m.log") +
                    (Y.app_state ? ", DOMAIN rep_app_state[r], rep_recv_dvc[r] or DOMAIN d.log" : ""));
    }
    fail(set, "a quantifier ranges over replicas, clients, Values, a..b, DOMAIN rep_log[r] or DOMAIN messages");
  }

  NodeP num_node(const NodeP& at, int v) const {
    NodeP kn = std::make_shared<Node>();
    kn->k = N_NUM; kn->v = v; kn->line = at->line; kn->col = at->col;
    return kn;
  }
  // Len(s)' = Len(s) /\ s'[i] = s[i] for the three positions (an absent entry equals an absent entry)
  void unchanged_seq(Seq q) {
    q.lp = true;
    seq_len(q);
    q.lp = false;
    seq_len(q);
    bin(W_EQ);
    for (int i = 1; i <= 3; i++) {
      const NodeP in = num_node(q.r, i);
      q.lp = true;
      seq_entry(q, in);
      q.lp = false;
      seq_entry(q, in);
      bin(W_EQ);
      bin(W_AND);
    }
  }
  // UNCHANGED e == (e' = e).  A whole per-replica variable unfolds over replicas.
  int compile_unchanged(const NodeP& n) {
    const NodeP& e = n->c[0];
    if (P) fail(n, "UNCHANGED inside a primed expression (it contains a prime itself)");
    if (AN) {                                                     // the analysis models: their own words and logs
      if (e->k == N_ID && !lookup(e->s) && !defs.count(e->s)) {
        refuse_absent(e, e->s);
        if (e->s == "messages")
          fail(e, "UNCHANGED messages: a whole bag is not a value that can be compared; quantify over DOMAIN messages and DOMAIN messages' instead");
        if (Y.app_state && e->s == "rep_recv_dvc")
          fail(e, std::string("UNCHANGED rep_recv_dvc: the sets of held DoViewChanges of ") + Y.spec +
                  " are not values that can be compared; compare Cardinality(rep_recv_dvc[r]) or quantify over rep_recv_dvc[r] and rep_recv_dvc'[r]");
        const struct { const char* name; int shift, width; } V[] = {{"rep_status", 0, 2}, {"rep_view_number", 2, 3}, {"rep_op_number", 5, 2}, {"rep_commit_number", 7, 2},
                                                                    {"rep_last_normal_view", 9, 3}, {"no_progress", Y.noprog_shift, 1}};
        for (const auto& v : V)
          if (e->s == v.name) {
            for (int r = 1; r <= M.R; r++) {
              P = true;
              ldbits(aword(r), v.shift, v.width);
              P = false;
              ldbits(aword(r), v.shift, v.width);
              bin(W_EQ);
              if (r > 1) bin(W_AND);
            }
            return TY_BOOL;
          }
        if (e->s == "rep_log" || (Y.app_state && e->s == "rep_app_state")) {
          for (int r = 1; r <= M.R; r++) {
            Seq q;
            q.kind = e->s == "rep_log" ? 1 : 2;
            q.r = num_node(e, r);
            unchanged_seq(q);
            if (r > 1) bin(W_AND);
          }
          return TY_BOOL;
        }
        static const char* const OTHER[] = {"rep_sent_dvc", "rep_sent_sv", "rep_peer_op_number", "aux_client_acked"};
        for (const char* o : OTHER)
          if (e->s == o)
            fail(e, "UNCHANGED " + e->s + ": a whole variable of " + Y.spec + " can be rep_status, rep_view_number, rep_op_number, rep_commit_number, rep_last_normal_view, rep_log, no_progress" +
                    (Y.app_state ? " or rep_app_state" : "") + "; apply UNCHANGED to an element otherwise");
      }
      Seq q;
      if (seq_of(e, &q) && (q.kind == 1 || q.kind == 2)) {        // UNCHANGED rep_log[r] / rep_app_state[r]: length and positions, still not a whole-log value
        if (q.lp) fail(e, "double prime: UNCHANGED of a primed log");
        unchanged_seq(q);
        return TY_BOOL;
      }
    }
    if (e->k == N_ID && !lookup(e->s) && !defs.count(e->s)) {
      static const struct { const char* name; int word, shift, width; } V[] = {{"rep_status", 0, 0, 2}, {"rep_view_number", 0, 2, 3}, {"rep_op_number", 0, 5, 2},
                                                                                 {"rep_commit_number", 0, 7, 2}, {"rep_last_normal_view", 0, 9, 3}, {"rep_log", 1, 0, 24}};
      for (const auto& v : V)
        if (e->s == v.name) {
          for (int r = 1; r <= M.R; r++) {
            P = true;
            ldbits(aword(r) + v.word, v.shift, v.width);
            P = false;
            ldbits(aword(r) + v.word, v.shift, v.width);
            bin(W_EQ);
            if (r > 1) bin(W_AND);
          }
          return TY_BOOL;
        }
      static const char* const OTHER[] = {"rep_sent_dvc", "rep_sent_sv", "rep_peer_op_number", "rep_client_table", "rep_svc_recv", "rep_dvc_recv", "aux_client_acked", "messages"};
      for (const char* o : OTHER)
        if (e->s == o)
          fail(e, "UNCHANGED " + e->s + ": a whole variable can be rep_status, rep_view_number, rep_op_number, rep_commit_number, rep_last_normal_view or rep_log; "
                  "apply UNCHANGED to an element otherwise");
    }
    bool lp = false;
    if (NodeP r = log_of(e, &lp)) {                             // UNCHANGED rep_log[r]: the whole log of one replica
      if (lp) fail(e, "double prime: UNCHANGED of a primed log");
      std::vector<int> vals;
      indexed({Ix{r, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& v) { ldbits(aword(v[0]) + 1, 0, 24); }, true);
      indexed({Ix{r, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& v) { ldbits(aword(v[0]) + 1, 0, 24); }, false);
      bin(W_EQ);
      return TY_BOOL;
    }
    P = true;
    const int a = compile(e);
    P = false;
    const int b = compile(e);
    if (a != b) fail(n, "UNCHANGED: the two sides have different types");
    bin(W_EQ);
    return TY_BOOL;
  }

  int compile(const NodeP& n) {
    switch (n->k) {
      case N_NUM: push((int)n->v); return TY_INT;
      case N_BOOL: push((int)n->v); return TY_BOOL;
      case N_NOT: want(n->c[0], compile(n->c[0]), TY_BOOL); emit(W_NOT, 0, 0); return TY_BOOL;
      case N_NEG: push(0); want(n->c[0], compile(n->c[0]), TY_INT); bin(W_SUB); return TY_INT;
      case N_QUANT: return compile_quant(n, 0);
      case N_PRIME: {                                           // e': every state variable inside e is the successor's; bound variables and constants are what they are
        if (P) fail(n, "double prime: a primed expression inside an expression that is primed");
        if (n->c[0]->k == N_ID && !lookup(n->c[0]->s) && !defs.count(n->c[0]->s)) {
          static const char* const FN[] = {"rep_status", "rep_view_number", "rep_op_number", "rep_commit_number", "rep_last_normal_view", "rep_sent_dvc", "rep_sent_sv",
                                           "rep_peer_op_number", "rep_client_table", "rep_log", "rep_svc_recv", "rep_dvc_recv", "aux_client_acked", "messages"};
          for (const char* e : FN)
            if (n->c[0]->s == e) fail(n, n->c[0]->s + "' is a function: apply it to an index");
          if (AN && (n->c[0]->s == "no_progress" || (Y.app_state && (n->c[0]->s == "rep_app_state" || n->c[0]->s == "rep_recv_dvc"))))
            fail(n, n->c[0]->s + "' is a function: apply it to an index");
        }
        P = true;
        const int t = compile(n->c[0]);
        P = false;
        return t;
      }
      case N_UNCHANGED: return compile_unchanged(n);
      case N_INDEX:
      case N_FIELD: return compile_path(n);
      case N_DOMAIN: fail(n, "DOMAIN is supported after \\in only (DOMAIN rep_log[r], DOMAIN messages, DOMAIN aux_client_acked)");
      case N_CALL: {
        const NodeP& a = n->c[0];
        int v;
        if (const_int(n, &v)) { push(v); return TY_INT; }
        if (AN) {
          Seq q;
          std::vector<Acc> acc;
          bool rp = false;
          NodeP root = flatten(a, acc);
          if (root->k == N_PRIME && root->c[0]->k == N_ID && root->c[0]->s == "rep_recv_dvc") root = strip_prime(root, &rp);
          if (n->s == "Len") {
            if (seq_of(a, &q)) { seq_len(q); return TY_INT; }
          } else if (Y.app_state && root->k == N_ID && root->s == "rep_recv_dvc" && !lookup(root->s) && !defs.count(root->s) && acc.size() == 1 && !acc[0].field) {
            std::vector<int> vals;
            indexed({Ix{acc[0].ix, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& r) {
              for (int s = 1; s <= M.R; s++) {
                ldbits(bword(r[0]), dvc_shift(s), 1);
                if (s > 1) bin(W_ADD);
              }
            }, P || rp);
            return TY_INT;
          }
          if (a->k == N_INDEX || a->k == N_FIELD || a->k == N_ID) compile(a);   // (an unknown or refused name says so itself)
          fail(n, std::string("Len of rep_log[r], m.log") + (Y.app_state ? ", rep_app_state[r], d.log; Cardinality(Values) and Cardinality(rep_recv_dvc[r])" : "; Cardinality(Values)") +
                      " are the supported forms");
        }
        if (n->s == "Len") {
          bool lp = false;
          NodeP r = log_of(a, &lp);
          if (!r) fail(n, "Len(rep_log[r]) is the supported form");
          emit_log_len(r, lp);
          return TY_INT;
        }
        std::vector<Acc> acc;
        bool rp = false;
        NodeP root = strip_prime(flatten(a, acc), &rp);
        const bool lp = P || rp;
        if (root->k == N_ID && !lookup(root->s) && acc.size() == 1 && !acc[0].field && (root->s == "rep_svc_recv" || root->s == "rep_dvc_recv")) {
          const bool svc = root->s == "rep_svc_recv";
          std::vector<int> vals;
          indexed({Ix{acc[0].ix, 1, M.R, TY_INT}}, 0, vals, -1, [&](const std::vector<int>& r) {
            if (svc) { ldbits(aword(r[0]), 14, M.R); emit(W_POPC, 0, 0); return; }
            for (int s = 1; s <= M.R; s++) {                   // x-slot s of the block: bit 0 = a DoViewChange from s is held
              ldbits(aword(r[0]) + 1 + (s >> 1), 32 * (s & 1), 1);
              if (s > 1) bin(W_ADD);
            }
          }, lp);
          return TY_INT;
        }
        fail(n, "Cardinality(Values), Cardinality(rep_svc_recv[r]) and Cardinality(rep_dvc_recv[r]) are the supported forms");
      }
      case N_ID: {
        const std::string& s = n->s;
        if (const Binding* b = lookup(s)) {
          if (b->kind == 2) fail(n, "a message is used through its fields (" + s + ".type, messages[" + s + "], ...)");
          if (b->kind == 3) fail(n, "a held DoViewChange is used through its fields (" + s + ".source, " + s + ".log[i], ...)");
          push(b->v);
          return b->kind == 1 ? TY_VALUE : TY_INT;
        }
        auto d = defs.find(s);
        if (d != defs.end()) {                                  // an earlier definition, inlined (nullary: it sees no bound variable)
          std::vector<Binding> saved;
          saved.swap(env);
          const int md = msg_depth;
          const int t = compile(d->second.body);
          msg_depth = md;
          env.swap(saved);
          return t;
        }
        if (s == compiling) fail(n, s + " refers to itself");
        int v;
        if (const_int(n, &v)) { push(v); return TY_INT; }
        if (AN) {
          refuse_absent(n, s);
          if (s == "StateTransfer") { push(2); return TY_STATUS; }  // vrst::ST2_STATETRANSFER
          if (s == "AnyDest") { push(7); return TY_INT; }           // vrst::ANYDEST: what m.dest reads; no replica has this number
          if (s == "no_progress_ctr") { ldbits(0, 20, 3); return TY_INT; }
          if (s == "no_progress" || (Y.app_state && (s == "rep_app_state" || s == "rep_recv_dvc"))) fail(n, s + " is a function: apply it to an index");
        }
        static const struct { const char* name; int code, type; } K[] = {
            {"Normal", ST_NORMAL, TY_STATUS}, {"ViewChange", ST_VIEWCHANGE, TY_STATUS}, {"Recovering", ST_RECOVERING, TY_STATUS},
            {"StartViewChangeMsg", T_SVC, TY_MTYPE}, {"PrepareMsg", T_PREPARE, TY_MTYPE}, {"PrepareOkMsg", T_PREPAREOK, TY_MTYPE},
            {"DoViewChangeMsg", T_DVC, TY_MTYPE}, {"StartViewMsg", T_SV, TY_MTYPE}, {"GetStateMsg", T_GETSTATE, TY_MTYPE},
            {"NewStateMsg", T_NEWSTATE, TY_MTYPE}, {"Nil", 0, TY_VALUE}};
        for (const auto& e : K)
          if (s == e.name) { push(e.code); return e.type; }
        if (value_literal(s)) {
          if (symmetry) fail(n, "the model value " + s + " cannot be named under SYMMETRY: bind a variable over Values instead");
          push(value_literal(s));
          return TY_VALUE;
        }
        if (s == "aux_svc") { ldbits(0, 8, 3); return TY_INT; }
        if (step) {                                             // not TLA+: the Next disjunct that produced the pair, and the names traces print
          if (s == "step_action") { emit(W_STEPACT, 0, +1); return TY_ACTION; }
          for (int a = 1; a < (int)A_COUNT; a++)                 // the action table's own names (vsr_model.hpp): the three specs name their disjuncts alike
            if (s == action_name(a)) { push(a); return TY_ACTION; }
        }
        static const char* const STATE[] = {"rep_status", "rep_view_number", "rep_op_number", "rep_commit_number", "rep_last_normal_view", "rep_sent_dvc", "rep_sent_sv",
                                            "rep_peer_op_number", "rep_client_table", "rep_log", "rep_svc_recv", "rep_dvc_recv", "aux_client_acked", "messages"};
        for (const char* e : STATE)
          if (s == e) fail(n, s + " is a function: apply it to an index");
        if (s == "replicas" || s == "clients" || s == "Values") fail(n, s + " is a set: it can be quantified over or tested with \\in");
        static const char* const UNLOWERED[] = {"aux_restart", "rep_rec_number", "rep_rec_recv", "RecoveryMsg", "RecoveryResponseMsg"};
        for (const char* e : UNLOWERED)
          if (s == e) fail(n, s + " belongs to the recovery protocol, which is not lowered");
        fail(n, "unknown identifier " + s + " (a definition must precede its use; a variable must be bound by \\A or \\E)");
      }
      case N_BIN: {
        const std::string& o = n->s;
        if (o == "/\\" || o == "\\/" || o == "=>" || o == "<=>") {
          want(n->c[0], compile(n->c[0]), TY_BOOL);
          want(n->c[1], compile(n->c[1]), TY_BOOL);
          bin(o == "/\\" ? W_AND : o == "\\/" ? W_OR : o == "=>" ? W_IMP : W_EQ);
          return TY_BOOL;
        }
        if (o == "+" || o == "-" || o == "\\div") {
          int v;
          if (const_int(n, &v)) { push(v); return TY_INT; }
          want(n->c[0], compile(n->c[0]), TY_INT);
          want(n->c[1], compile(n->c[1]), TY_INT);
          bin(o == "+" ? W_ADD : o == "-" ? W_SUB : W_DIV);
          return TY_INT;
        }
        if (o == "=" || o == "#") {
          const int a = compile(n->c[0]), b = compile(n->c[1]);
          if (a != b) fail(n, std::string("type mismatch: ") + type_name(a) + " is compared with " + type_name(b));
          bin(o == "=" ? W_EQ : W_NE);
          return TY_BOOL;
        }
        if (o == "<" || o == "<=" || o == ">" || o == ">=") {
          want(n->c[0], compile(n->c[0]), TY_INT);
          want(n->c[1], compile(n->c[1]), TY_INT);
          bin(o == "<" ? W_LT : o == "<=" ? W_LE : o == ">" ? W_GT : W_GE);
          return TY_BOOL;
        }
        if (o == "\\in") {
          const NodeP& set = n->c[1];
          int lo, hi, kind;
          NodeP logr;
          bool domp = false, loglp = false;
          const NodeP dom = set->k == N_DOMAIN ? strip_prime(set->c[0], &domp) : nullptr;
          if (dom && dom->k == N_ID && dom->s == "aux_client_acked" && !lookup("aux_client_acked")) {
            std::vector<int> vals;
            indexed({Ix{n->c[0], 1, M.n, TY_VALUE}}, 0, vals, 0, [&](const std::vector<int>& v) { ldbits(0, 11 + 2 * (v[0] - 1), 2); push(0); bin(W_NE); }, P || domp);
            return TY_BOOL;
          }
          if (dom && dom->k == N_ID && dom->s == "messages" && !lookup("messages"))
            fail(set, "\\in DOMAIN messages as a test would search the bag: quantify over it instead (a message of one bag cannot be looked up in the other)");
          Seq q;
          if (AN && set->k == N_DOMAIN && seq_of(set->c[0], &q)) {      // i \in DOMAIN s  ==  entry i of s is there (out of 1..3: the absent entry)
            seq_entry(q, n->c[0]);
            push(0);
            bin(W_NE);
            return TY_BOOL;
          }
          if (const_set(set, &lo, &hi, &kind)) {
            want(n->c[0], compile(n->c[0]), kind ? TY_VALUE : TY_INT);
            push(lo); bin(W_GE);
            compile(n->c[0]);
            push(hi); bin(W_LE);
            bin(W_AND);
            return TY_BOOL;
          }
          if (set->k == N_DOMAIN && (logr = log_of(set->c[0], &loglp))) {
            want(n->c[0], compile(n->c[0]), TY_INT);
            push(1); bin(W_GE);
            compile(n->c[0]);
            emit_log_len(logr, loglp);
            bin(W_LE);
            bin(W_AND);
            return TY_BOOL;
          }
          if (AN) {
            const NodeP inner = set->k == N_DOMAIN ? set->c[0] : set;
            if (inner->k == N_INDEX || inner->k == N_FIELD) compile(inner);
            fail(set, "\\in is supported for replicas, Values, a..b, DOMAIN aux_client_acked and the domain of a log (rep_log[r], m.log, ...)");
          }
          fail(set, "\\in is supported for replicas, clients, Values, a..b, DOMAIN rep_log[r] and DOMAIN aux_client_acked");
        }
        if (o == "..") fail(n, "a range can be quantified over or tested with \\in");
        fail(n, "operator " + o + " is not supported");
      }
    }
    fail(n, "unsupported expression");
  }
};

}  // namespace where_detail

// 0 = compiled; 1 = refused (VSRMC_E_ARG), 2 = beyond a cap (VSRMC_E_REP): *err says why
inline int where_compile(const Model& M, bool symmetry, const std::vector<std::string>& value_names, const std::string& text, WhereProgram* out, std::string* err,
                         bool step = false) {
  using namespace where_detail;
  *out = WhereProgram();
  try {
    Parser P;
    P.step = step;
    P.t = lex(text);
    Compiler C(M, symmetry, value_names, *out);
    C.step = step;
    bool has_defs = false;
    for (const Tok& k : P.t) has_defs = has_defs || (k.kind == TK_OP && k.s == "==");
    auto export_top = [&](const std::string& name, const Tok& at) {
      if (out->names.size() >= (size_t)WHERE_MAX_EXPORTS) fail_at(at.line, at.col, "more than 8 exported definitions (write LOCAL Name == ... for a helper)");
      C.emit(W_OUT, (u32)out->names.size(), -1);
      out->names.push_back(name);
    };
    if (!has_defs) {
      const Tok first = P.peek();
      NodeP e = P.expr(1);
      if (P.peek().kind != TK_EOF) P.fail(P.peek(), "unexpected '" + P.peek().s + "' after the expression");
      C.want(e, C.compile(e), TY_BOOL);
      export_top("where", first);
    } else {
      while (P.peek().kind != TK_EOF) {
        bool local = false;
        if (P.is_id("LOCAL")) { local = true; P.p++; }
        const Tok name = P.peek();
        if (name.kind != TK_ID || !P.is_op("==", 1)) P.fail(name, "expected a definition: Name == expression");
        if (C.defs.count(name.s)) P.fail(name, name.s + " is defined twice");
        P.p += 2;
        NodeP e = P.expr(1);
        if (local) {                                            // type-checked where it is used; checked here too, its code discarded
          WhereProgram scratch;
          Compiler T(M, symmetry, value_names, scratch);
          T.step = step;
          T.defs = C.defs;
          T.compiling = name.s;
          T.compile(e);
        } else {
          C.compiling = name.s;
          C.want(e, C.compile(e), TY_BOOL);
          C.compiling.clear();
          export_top(name.s, name);
        }
        C.defs[name.s] = Def{e};
      }
      if (out->names.empty()) fail_at(1, 1, "no exported definition");
    }
    C.emit(W_END, 0, 0);
    out->step = step;
  } catch (const Err& e) {
    *err = e.msg;
    *out = WhereProgram();
    return e.code;
  }
  return 0;
}

}  // namespace vsr
