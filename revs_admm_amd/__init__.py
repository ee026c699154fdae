"""revs_admm_amd -- MI355X-native engine for the distributed (ADMM) path of REVS.

    lpsolver       the reference's call surface (solve_ADMM, solve_residence, compute_Rmat)
    revs_fixture   REVS class (read_inputs / get_*_optimal) over the engine
    engine         array-level AdmmEngine: device buffers + kernel driver
    network        AdmmEngine.network_report: line flows / loading, node voltages and their box-plot numbers
    baselines      rule schedules: uncontrolled / last-minute / trickle charging from the residence records
    load_profile   the demand curve of a schedule: load per slot by class of residence, peaks, load factor, diversity
    charging       what the chargers do: ChargingReport, charging_report / charging_report_device -- sessions, waits,
                   chargers on per slot, state of charge at departure and cost per EV
    headroom       AdmmEngine.headroom_report: spare charger power per node and slot, and what limits it
    losses         AdmmEngine.loss_report: line losses, marginal loss per node, the day's lost energy and its cost
    attribution    AdmmEngine.attribution_report: which nodes' load causes the worst node's voltage drop, and the EVs'
                   part of it: AttributionReport, attribution_report_device
    risk           AdmmEngine.risk_report: the odds of undervoltage per node and slot when the net load is a forecast
                   with independent and shared errors: RiskReport, risk_report_device
    prices         AdmmEngine.price_report: nodal prices (energy, marginal loss, congestion) from the voltage rows'
                   multipliers, the rent every line collects and what reinforcing it would save: PriceReport,
                   price_report_device
    powerflow      AdmmEngine.powerflow_report: the nonlinear branch-flow voltages, flows and losses beside the linear
                   model's, and the undervoltages the linear model misses: PowerFlowReport, powerflow_report_device
    transformers   AdmmEngine.transformer_report: the service transformers' loading, hot-spot and loss of life
    flexibility    how much charging can still be moved: FlexReport, flexibility_report / flexibility_report_device -- up and
                   down reserve per EV, node and slot, the slot a car is ready at and the slack it leaves
    drawing        the reference's compute_flows / compute_voltage / compute_losses over it (no figures)
    synthetic      synthetic feeders / residences for benchmarks and tests
    build          compiles csrc/*.hip into librevs_admm.so (gfx950)

Importing the package does not need a GPU; computing anything does.
"""
__version__ = "0.1.0"
